#!/usr/bin/env python3
"""Measure ray accumulators (pt_accum_create_rays: k_render_rays_list; dev tool;
prints one JSON document and writes it to --out, default
profiles/rays_adaptive_k2.json, stamped with pt_build_id).

    python3 scripts/bench_rays_adaptive.py [--parts a,b,c] [--out FILE]
    python3 scripts/bench_rays_adaptive.py --parts parent --parent-root DIR [--rounds 5]

Kernel times are HIP events (pt_last_kernel_ms), one process, the legs
alternating, --launches launches each (default 12), the median of the last
--keep (default 8).
  a       all 64 samples of the K2 frame's own rays (Cornell 512x512, 4 bounces,
          seed 9; cameras.scene_camera_rays in image order) in one pass of the
          ray list kernel (min = max = step = 64 on a 512 x 512 ray accumulator)
          against k_render_rays with S and Q on the same records, the frame
          list kernel (the same rule on a frame accumulator) and k_render; and
          whether the ray accumulator's S, Q are the frame accumulator's bits
  b       whole runs at tol 0.05 and 0.02 (min 8, step 8, budget 64) on those
          rays and on the look-at frame from (2, 1.5, 3) of
          scripts/bench_rays.py (profiles/rays_k2.json): samples taken, passes, the passes' kernel
          time and the whole run's wall time (selects and reads included),
          against the frame accumulator on the scene's own camera
  c       the K5 synth mesh (100k triangles, 512x512, 4 bounces) at budget 16
          through the single list kernel: one pass of 16 against k_render_rays
          with S and Q under PT_FLAG_RAYS_SINGLE and the frame list kernel under
          PT_FLAG_MEGAKERNEL, and the tol-0.05 run (min 8, step 8)
  parent  `python bench.py --gpus 1` and `--config k5` on this tree and on the
          parent commit's (DIR: a built checkout of it) in alternating child
          processes, --rounds pairs each, written to --out-parent (default
          profiles/rays_adaptive_parent.json; scripts/bench_lens.py
          part_parent_k5)"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from bench_aa import stat  # noqa: E402
from bench_lens import part_parent_k5  # noqa: E402
from bench_rays import RayLegs, time_legs  # noqa: E402

W = H = 512
BUDGET, BOUNCES, SEED = 64, 4, 9
LOOK = dict(eye=(2.0, 1.5, 3.0), target=(0.0, 0.0, -24.0), up=(0.0, 1.0, 0.0), fov_y=30.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="a,b,c")
    ap.add_argument("--launches", type=int, default=12)
    ap.add_argument("--keep", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5, help="part parent: pairs of child processes per config")
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rays_adaptive_k2.json"))
    ap.add_argument("--out-parent", default=os.path.join(ROOT, "profiles", "rays_adaptive_parent.json"))
    args = ap.parse_args()
    parts = args.parts.split(",")
    if "parent" in parts:
        if not args.parent_root:
            raise SystemExit("--parts parent needs --parent-root")
        args.configs, args.order = "k2,k5", "parent,new"
        write(args.out_parent, {"bench_parent": part_parent_k5(args)})
        parts.remove("parent")
    if not parts:
        return
    res = {}
    if os.path.exists(args.out):   # (parts measured earlier stay)
        with open(args.out) as f:
            res = json.load(f)
    import torch
    torch.cuda.set_device(0)
    from pathtracerpython_amd import _native
    res.update(build_id=_native.build_id(), device=torch.cuda.get_device_name(0), launches=args.launches,
               keep=args.keep)
    for name, fn in (("a", part_a), ("b", part_b), ("c", part_c)):
        if name in parts:
            res[name] = fn(args)
    write(args.out, res)


def write(path, doc):
    text = json.dumps(doc, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write(text + "\n")
    print(text)


def cornell():
    from pathtracerpython_amd import scene_reader
    scene_reader.VERBOSE = False
    return scene_reader.Scene(os.path.join(ROOT, "scenes", "cornell", "cornellroom.sdl"))


def frame_records(scene, w, h):
    """The frame's own rays as image-order records (o, d, keys)."""
    from pathtracerpython_amd import cameras
    return cameras.to_image_order(*cameras.scene_camera_rays(scene, w, h), w, h)


def one_pass(acc, p, adapt):
    """A launcher of one whole-budget pass from an empty accumulator."""
    def go():
        acc.reset()
        acc.render(p, adapt)
    return go


def uniform_legs(args, r, scene, w, h, spp, single):
    """One pass of spp samples through the ray list kernel, k_render_rays with
    the moments, the frame list kernel and k_render, alternating.  single: the
    single-kernel flags of a scene with a BVH."""
    import torch
    from pathtracerpython_amd._abi import PT_FLAG_RAYS_SINGLE, make_adapt, with_flags
    from pathtracerpython_amd.adaptive import Accumulator, RayAccumulator
    o, d, k = frame_records(scene, w, h)
    adapt = make_adapt(0.0, spp, spp, spp, 0.01)
    pa = r.params(w, h, spp, BOUNCES, SEED, megakernel=single)
    pray = r.params(w, h, spp, BOUNCES, SEED)
    pf = r.params(w, h, spp, BOUNCES, SEED, out_f64=True, megakernel=single)
    pr = r.params(1, 1, spp, BOUNCES, SEED, out_f64=True)
    if single:
        pr = with_flags(pr, PT_FLAG_RAYS_SINGLE)
    fb = torch.empty((h, w, 3), dtype=torch.float64, device="cuda")
    legs = RayLegs(r, scene, w, h)
    with RayAccumulator(r, o, d, k, (h, w)) as racc, Accumulator(r, w, h) as facc:
        t = time_legs(args, {
            "k_render_rays_list": (one_pass(racc, pray, adapt), r),
            "k_render_rays_moments": (lambda: legs.launch(pr, True), r),
            "k_render_list": (one_pass(facc, pa, adapt), r),
            "k_render": (lambda: r.render_device(pf, fb.data_ptr(), 0), r)})
        one_pass(racc, pray, adapt)()
        torch.cuda.synchronize()
        info = r.last_launch()
        a, b = racc.read(S=True, Q=True, n=True), facc.read(S=True, Q=True, n=True)
        one_pass(facc, pa, adapt)()
        torch.cuda.synchronize()
        finfo = r.last_launch()
    med = {x: v["median"] for x, v in t.items()}
    return {"kernel_ms": t, "lanes_per_record": info["lanes_per_pixel"], "frame_lanes_per_pixel": finfo["lanes_per_pixel"],
            "ratio_rays_list_to_k_render_rays_moments": med["k_render_rays_list"] / med["k_render_rays_moments"],
            "ratio_rays_list_to_k_render_list": med["k_render_rays_list"] / med["k_render_list"],
            "ratio_k_render_list_to_k_render": med["k_render_list"] / med["k_render"],
            "ratio_rays_list_to_k_render": med["k_render_rays_list"] / med["k_render"],
            "msamples_per_s_rays_list": w * h * spp / med["k_render_rays_list"] / 1e3,
            "same_bits_as_the_frame_accumulator": bool(
                info["lanes_per_pixel"] == finfo["lanes_per_pixel"] and
                all(np.array_equal(a[x].view(np.uint64) if x != "n" else a[x],
                                   b[x].view(np.uint64) if x != "n" else b[x]) for x in ("S", "Q", "n")))}


def whole_run(r, make_acc, p, adapt, reps):
    """An adaptive run, reps times: samples, passes, the passes' kernel ms
    (HIP events, summed) and the run's wall ms (selects and the closing read
    included), each the median."""
    import torch
    from pathtracerpython_amd.adaptive import run_passes
    kern, wall, passes = [], [], None
    for _ in range(reps):
        with make_acc() as acc:
            torch.cuda.synchronize()
            ms = []
            t0 = time.perf_counter()
            passes = run_passes(acc, p, adapt, on_pass=lambda *_: ms.append(r.last_kernel_ms()))
            acc.read(S=True, n=True)
            wall.append((time.perf_counter() - t0) * 1e3)
            kern.append(sum(ms))
    return {"samples": int(sum(k for _, k in passes)), "passes": len(passes), "list_lengths": [a for a, _ in passes],
            "pass_kernel_ms": stat(kern), "wall_ms": stat(wall)}


def adaptive_rows(r, scene, w, h, budget, recs, reps, tols=(0.05, 0.02), single=False):
    """The runs of part b / c: recs name -> image-order records, and the frame
    accumulator on the scene's own camera."""
    from pathtracerpython_amd._abi import make_adapt
    from pathtracerpython_amd.adaptive import Accumulator, RayAccumulator
    rows = []
    for tol in tols:
        adapt = make_adapt(tol, budget, 8, 8, 0.01)
        row = {"tol": tol, "min_spp": 8, "step_spp": 8, "floor": 0.01, "budget": budget,
               "uniform_samples": w * h * budget}
        for name, (o, d, k) in recs.items():
            x = whole_run(r, lambda: RayAccumulator(r, o, d, k, (h, w)), r.params(w, h, budget, BOUNCES, SEED),
                          adapt, reps)
            x["fraction_of_uniform"] = x["samples"] / (w * h * budget)
            row["rays_" + name] = x
        x = whole_run(r, lambda: Accumulator(r, w, h), r.params(w, h, budget, BOUNCES, SEED, megakernel=single),
                      adapt, reps)
        x["fraction_of_uniform"] = x["samples"] / (w * h * budget)
        row["frame_accumulator"] = x
        if "frame" in recs:
            row["ratio_rays_frame_to_frame_accumulator_kernel"] = (row["rays_frame"]["pass_kernel_ms"]["median"] /
                                                                   x["pass_kernel_ms"]["median"])
            row["ratio_rays_frame_to_frame_accumulator_wall"] = (row["rays_frame"]["wall_ms"]["median"] /
                                                                 x["wall_ms"]["median"])
        rows.append(row)
    return rows


def part_a(args):
    from pathtracerpython_amd.render import Renderer
    sc = cornell()
    with Renderer(sc) as r:
        out = uniform_legs(args, r, sc, W, H, BUDGET, False)
    out["shape"] = {"width": W, "height": H, "spp": BUDGET, "bounces": BOUNCES, "seed": SEED}
    return out


def part_b(args):
    from pathtracerpython_amd import cameras
    from pathtracerpython_amd.render import Renderer
    sc = cornell()
    look = cameras.to_image_order(*cameras.look_at_rays(LOOK["eye"], LOOK["target"], LOOK["up"], LOOK["fov_y"], W, H),
                                  W, H)
    lo, hi = cameras.rays_box(np.array([LOOK["eye"], [float(v) for v in sc.eye]]))
    with Renderer(sc, ray_box=(lo, hi)) as r:
        rows = adaptive_rows(r, sc, W, H, BUDGET, {"frame": frame_records(sc, W, H), "look_at": look},
                             max(3, args.keep // 2))
    return {"shape": {"width": W, "height": H, "budget": BUDGET, "bounces": BOUNCES, "seed": SEED,
                      "look_at": {k: list(v) if isinstance(v, tuple) else v for k, v in LOOK.items()}},
            "runs": rows}


def part_c(args):
    import tempfile
    from pathtracerpython_amd import scene_reader
    from pathtracerpython_amd.render import Renderer
    from pathtracerpython_amd.synth import write_k5_scene
    scene_reader.VERBOSE = False
    k5 = scene_reader.Scene(write_k5_scene(tempfile.mkdtemp(), n_tris=100_000, seed=0, size=W))
    with Renderer(k5) as r:
        out = uniform_legs(args, r, k5, W, H, 16, True)
        out["runs"] = adaptive_rows(r, k5, W, H, 16, {"frame": frame_records(k5, W, H)}, 3, tols=(0.05,), single=True)
    out["shape"] = {"scene": "K5 synth", "n_tris": 100_000, "width": W, "height": H, "budget": 16, "bounces": BOUNCES,
                    "seed": SEED}
    return out


if __name__ == "__main__":
    main()
