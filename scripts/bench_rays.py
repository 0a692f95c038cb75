#!/usr/bin/env python3
"""Measure the ray kernels (pt_radiance: k_render_rays and the wavefront ray
form; dev tool; prints one JSON document and writes it to --out, default
profiles/rays_k2.json, stamped with pt_build_id).

    python3 scripts/bench_rays.py [--parts kernel,k5] [--out FILE]
    python3 scripts/bench_rays.py --parts kernel,k5,parent --parent-root DIR [--rounds 5]

Kernel times are HIP events (pt_last_kernel_ms), one process, the legs
alternating, --launches launches each (default 20), the median of the last
--keep (default 10).
  kernel  the K2 frame (Cornell 512x512, 64 spp, 4 bounces, seed 9) three ways
          on one scene handle: k_render, k_render_lens (lens R = 0.25,
          zf = -24) and k_render_rays on the frame's own rays
          (cameras.scene_camera_rays, device arrays), at the library's lane
          count, with and without the moments; and whether the ray frame is
          k_render's bit for bit at a fixed lane count
  k5      a scene with a BVH (synth.write_k5_scene, 100k triangles, seed 0,
          512x512, 16 spp, 4 bounces), written to --out-k5 (default
          profiles/rays_k5.json): the frame's rays through (a) the single ray
          kernel (PT_FLAG_RAYS_SINGLE), (b) the wavefront ray form, (c) the
          frame through the wavefront kernels, (d) (b) with the moments, and
          the frame through the single kernel; (a) and (b) again on a
          look_at_rays camera from an in-box origin, on that batch with every
          fourth origin outside the frame, and on a batch of 1,024 rays
  parent  `python bench.py --gpus 1` on this tree and on the parent commit's
          (DIR: a built checkout of it) in alternating child processes,
          --rounds each, then once more with the order swapped
          (scripts/bench_lens.py part_parent_k5)"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from bench_aa import stat  # noqa: E402
from bench_lens import part_parent_k5  # noqa: E402

W = H = 512
SPP, BOUNCES, SEED = 64, 4, 9
LENS = (0.25, -24.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="kernel,k5")
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--keep", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5, help="part parent: child processes per tree and order")
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rays_k2.json"))
    ap.add_argument("--out-k5", default=os.path.join(ROOT, "profiles", "rays_k5.json"))
    args = ap.parse_args()
    parts = args.parts.split(",")
    res = {}
    if os.path.exists(args.out):   # (parts measured earlier stay)
        with open(args.out) as f:
            res = json.load(f)
    if "kernel" in parts:
        res["kernel"] = part_kernel(args)
    if "k5" in parts:   # (a document of its own; rays_k2.json keeps the figures of the commit before)
        text = json.dumps({"k5": part_k5(args)}, indent=1)
        os.makedirs(os.path.dirname(os.path.abspath(args.out_k5)), exist_ok=True)
        with open(args.out_k5, "w") as f:
            f.write(text + "\n")
        print(text)
        if parts == ["k5"]:
            return
    if "parent" in parts:
        if not args.parent_root:
            raise SystemExit("--parts parent needs --parent-root")
        args.configs = "k2"
        rows = {}
        for order in ("parent,new", "new,parent"):
            args.order = order
            rows["order " + order.replace(",", ", ")] = part_parent_k5(args)
        res["bench_parent"] = rows
    text = json.dumps(res, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)


class RayLegs:
    """The frame's rays of a renderer on the device, and launches of
    pt_radiance_device on them."""

    def __init__(self, r, scene, w, h):
        import torch
        from pathtracerpython_amd import cameras
        from pathtracerpython_amd._abi import make_rays
        self.r, self.n, self.w, self.h = r, w * h, w, h
        rec = make_rays(*cameras.scene_camera_rays(scene, w, h))
        self.rays = torch.from_numpy(np.frombuffer(rec.tobytes(), dtype=np.uint8).copy()).cuda()
        self.rgb = torch.empty((self.n, 3), dtype=torch.float64, device="cuda")
        self.S, self.Q = torch.empty_like(self.rgb), torch.empty_like(self.rgb)

    def launch(self, p, moments=False):
        from pathtracerpython_amd import _native
        _native.check(self.r._lib.pt_radiance_device(
            self.r._h, C.c_void_p(self.rays.data_ptr()), self.n, C.byref(p), C.c_void_p(self.rgb.data_ptr()),
            C.c_void_p(self.S.data_ptr()) if moments else None, C.c_void_p(self.Q.data_ptr()) if moments else None,
            None), "pt_radiance_device")

    def image(self):
        from pathtracerpython_amd import cameras
        return np.ascontiguousarray(cameras.rays_to_image(self.rgb.cpu().numpy(), self.w, self.h))


def time_legs(args, legs):
    """legs: name -> callable launching once; alternating; (stats, last launch info)."""
    import torch
    ms = {k: [] for k in legs}
    for _ in range(args.launches):
        for k, (fn, r) in legs.items():
            fn()
            torch.cuda.synchronize()
            ms[k].append(r.last_kernel_ms())
    return {k: stat(v[-args.keep:]) for k, v in ms.items()}


def part_kernel(args):
    import torch
    torch.cuda.set_device(0)
    from pathtracerpython_amd import _native, scene_reader
    from pathtracerpython_amd.render import Renderer
    scene_reader.VERBOSE = False
    sc = scene_reader.Scene(os.path.join(ROOT, "scenes", "cornell", "cornellroom.sdl"))
    out = {"shape": {"width": W, "height": H, "spp": SPP, "bounces": BOUNCES, "seed": SEED,
                     "lens": {"radius": LENS[0], "focus_z": LENS[1]}},
           "build_id": _native.build_id(), "device": torch.cuda.get_device_name(0), "launches": args.launches,
           "keep": args.keep}
    with Renderer(sc, lens=LENS) as r:   # (the lens scene's records for all three, as profiles/lens_k2.json)
        fb = torch.empty((H, W, 3), dtype=torch.float64, device="cuda")
        legs = RayLegs(r, sc, W, H)
        pf = r.params(W, H, SPP, BOUNCES, SEED, out_f64=True, lens=False)
        pl = r.params(W, H, SPP, BOUNCES, SEED, out_f64=True)
        pr = r.params(1, 1, SPP, BOUNCES, SEED, out_f64=True, lens=False)
        t = time_legs(args, {
            "k_render": (lambda: r.render_device(pf, fb.data_ptr(), 0), r),
            "k_render_lens": (lambda: r.render_device(pl, fb.data_ptr(), 0), r),
            "k_render_rays": (lambda: legs.launch(pr), r),
            "k_render_rays_moments": (lambda: legs.launch(pr, True), r)})
        legs.launch(pr)
        torch.cuda.synchronize()
        lanes = r.last_launch()["lanes_per_pixel"]
        out["kernel_ms"] = t
        out["lanes_per_record"] = lanes
        med = {k: v["median"] for k, v in t.items()}
        out["ratio_rays_to_k_render"] = med["k_render_rays"] / med["k_render"]
        out["ratio_rays_to_k_render_lens"] = med["k_render_rays"] / med["k_render_lens"]
        out["ratio_rays_moments_to_rays"] = med["k_render_rays_moments"] / med["k_render_rays"]
        out["msamples_per_s_rays"] = W * H * SPP / med["k_render_rays"] / 1e3
        # the ray frame against the frame: bit for bit below k_render's tail rows
        # (its top sixteenth of rows gets more lanes), ~1e-15 relative there
        r.render_device(pf, fb.data_ptr(), 0)
        torch.cuda.synchronize()
        frame, rays = fb.cpu().numpy(), legs.image()
        info = r.last_launch()
        tail = (H + 15) // 16
        out["frame_lanes_per_pixel"] = info["lanes_per_pixel"]
        out["same_bits_below_the_tail_rows"] = bool(lanes == info["lanes_per_pixel"] and
                                                    np.array_equal(frame[tail:].view(np.uint64),
                                                                   rays[tail:].view(np.uint64)))
        out["max_abs_difference_whole_frame"] = float(np.abs(frame - rays).max())
    return out


def part_k5(args):
    import tempfile
    import torch
    torch.cuda.set_device(0)
    from pathtracerpython_amd import _native, cameras, scene_reader
    from pathtracerpython_amd._abi import PATH_NAMES, PT_FLAG_RAYS_SINGLE, make_rays, with_flags
    from pathtracerpython_amd.render import Renderer
    from pathtracerpython_amd.synth import write_k5_scene
    scene_reader.VERBOSE = False
    Wb = Hb = 512
    spp, bounces = 16, 4
    k5 = scene_reader.Scene(write_k5_scene(tempfile.mkdtemp(), n_tris=100_000, seed=0, size=Wb))
    out = {"shape": {"scene": "K5 synth", "n_tris": 100_000, "width": Wb, "height": Hb, "spp": spp,
                     "bounces": bounces, "seed": SEED},
           "build_id": _native.build_id(), "device": torch.cuda.get_device_name(0),
           "launches": args.launches, "keep": args.keep}

    def run(r, legs):
        """{name: {kernel_ms, path, lanes_per_pixel, steps}} of the legs, alternating."""
        info = {}

        def leg(name, fn):
            def go():
                fn()
                info[name] = r.last_launch()
            return go, r
        t = time_legs(args, {k: leg(k, fn) for k, fn in legs.items()})
        return {k: {"kernel_ms": t[k], "path": PATH_NAMES[info[k]["path"]],
                    "lanes_per_pixel": info[k]["lanes_per_pixel"], "steps": info[k]["steps"]} for k in t}

    def spread(x):
        return x["kernel_ms"]["max"] - x["kernel_ms"]["min"]

    def pair(r, legs):
        """(a) the single ray kernel and (b) the wavefront ray form on one batch."""
        pr = r.params(1, 1, spp, bounces, SEED, out_f64=True)
        ps = with_flags(pr, PT_FLAG_RAYS_SINGLE)
        res = run(r, {"rays_single_kernel": lambda: legs.launch(ps), "rays_wavefront": lambda: legs.launch(pr)})
        res["ratio_wavefront_to_single_kernel"] = (res["rays_wavefront"]["kernel_ms"]["median"] /
                                                   res["rays_single_kernel"]["kernel_ms"]["median"])
        return res

    # the frame's own rays on the plain scene: (a) the single ray kernel, (b) the
    # wavefront ray form, (c) the frame through the wavefront kernels, (d) (b)
    # with the moments; and the frame through the single kernel, for the ratio
    # of k_render_rays to k_render
    with Renderer(k5) as r:
        fb = torch.empty((Hb, Wb, 3), dtype=torch.float64, device="cuda")
        legs = RayLegs(r, k5, Wb, Hb)
        pm = r.params(Wb, Hb, spp, bounces, SEED, out_f64=True, megakernel=True)
        pw = r.params(Wb, Hb, spp, bounces, SEED, out_f64=True)
        pr = r.params(1, 1, spp, bounces, SEED, out_f64=True)
        ps = with_flags(pr, PT_FLAG_RAYS_SINGLE)
        t = run(r, {"rays_single_kernel": lambda: legs.launch(ps),
                    "rays_wavefront": lambda: legs.launch(pr),
                    "frame_wavefront": lambda: r.render_device(pw, fb.data_ptr(), 0),
                    "rays_wavefront_moments": lambda: legs.launch(pr, True),
                    "frame_single_kernel": lambda: r.render_device(pm, fb.data_ptr(), 0)})
        out["frame_rays"] = t
        med = {k: v["kernel_ms"]["median"] for k, v in t.items()}
        out["ratio_rays_wavefront_to_rays_single_kernel"] = med["rays_wavefront"] / med["rays_single_kernel"]
        out["ratio_rays_wavefront_to_frame_wavefront"] = med["rays_wavefront"] / med["frame_wavefront"]
        out["ratio_rays_single_kernel_to_frame_single_kernel"] = med["rays_single_kernel"] / med["frame_single_kernel"]
        out["ratio_moments_to_rays_wavefront"] = med["rays_wavefront_moments"] / med["rays_wavefront"]
        out["largest_spread_of_a_leg_ms"] = max(spread(v) for v in t.values())
        out["wavefront_faster_than_single_kernel_by_more_than_the_spread"] = bool(
            med["rays_single_kernel"] - med["rays_wavefront"] > out["largest_spread_of_a_leg_ms"])
        # the three results of the frame agree
        r.render_device(pw, fb.data_ptr(), 0)
        torch.cuda.synchronize()
        frame = fb.cpu().numpy()
        legs.launch(pr)
        torch.cuda.synchronize()
        wf = legs.image()
        legs.launch(ps)
        torch.cuda.synchronize()
        out["rays_wavefront_equals_rays_single_kernel_bitwise"] = bool(
            np.array_equal(wf.view(np.uint64), legs.image().view(np.uint64)))
        out["max_abs_difference_to_the_frame"] = float(np.abs(frame - wf).max())
        # a small batch (1,024 of the frame's rays, evenly strided) both ways
        small = RayLegs(r, k5, Wb, Hb)
        small.rays = small.rays.view(Wb * Hb, 56)[::Wb * Hb // 1024].contiguous().view(-1)
        small.n = 1024
        out["small_batch_1024"] = pair(r, small)
    # a free camera: look_at_rays from an in-box origin other than the eye, the
    # scene made with the box of the eye and that origin; and the same batch with
    # every fourth origin moved outside the frame (the f64 primary's price)
    eye2 = (2.0, 1.5, 3.0)
    o, d, keys = cameras.look_at_rays(eye2, (0.0, 0.0, -24.0), (0.0, 1.0, 0.0), 30.0, Wb, Hb)
    lo, hi = cameras.rays_box(np.array([eye2, [float(v) for v in k5.eye]]))
    with Renderer(k5, ray_box=(lo, hi)) as r:
        legs = RayLegs(r, k5, Wb, Hb)
        legs.rays = torch.from_numpy(np.frombuffer(make_rays(o, d, keys).tobytes(), dtype=np.uint8).copy()).cuda()
        out["look_at"] = dict(pair(r, legs), origin=list(eye2))
        o4 = o.copy()
        o4[::4, 2] += 200.0   # far beyond the box, along +z: the direction still faces the room
        legs.rays = torch.from_numpy(np.frombuffer(make_rays(o4, d, keys).tobytes(), dtype=np.uint8).copy()).cuda()
        out["look_at_every_fourth_origin_outside"] = pair(r, legs)
    return out


if __name__ == "__main__":
    main()
