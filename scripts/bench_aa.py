#!/usr/bin/env python3
"""Measure antialiasing (PT_FLAG_AA; dev tool; prints one JSON document and
writes it to --out, default profiles/aa_k2.json, stamped with pt_build_id).

    python3 scripts/bench_aa.py [--parts uniform,list,effect,bvh] [--out FILE]
    python3 scripts/bench_aa.py --parts k5            (writes profiles/aa_k5.json)
    python3 scripts/bench_aa.py --parts parent --parent-root DIR [--rounds 5]

The K2 frame: Cornell 512x512, 64 spp, 4 bounces, seed 9.  Kernel times are
HIP events (pt_last_kernel_ms), one process, the legs alternating, --launches
launches each (default 20), the median of the last --keep (default 10).
  uniform  k_render_aa beside k_render: the ratio is the price of antialiasing
  list     k_render_list_aa beside k_render_list: all 64 samples through the
           list (one pass of 64), and the tol-0.05 adaptive run (min 8, step 8,
           floor 0.01): summed pass kernel time, wall time, samples, passes, and
           how the count map moved (edge pixels: a 3x3 neighbourhood of the
           first-hit object that is not constant)
  effect   Cornell 64x64: RMSE of a 64-spp antialiased frame and of a 64-spp
           centre-ray frame against a 4096-spp antialiased frame of another
           seed, over the edge pixels and over the rest
  bvh      a scene with a BVH (synth.write_k5_scene, 100k triangles, 512x512,
           16 spp, 4 bounces): the antialiased single kernel beside the
           centre-ray single kernel (megakernel=True) and the wavefront render
  k5       the same scene and shape, antialiasing through the wavefront kernels
           (the default on BVH scenes) beside the antialiased single kernel
           (megakernel=True) and the centre-ray wavefront render; one
           PT_FLAG_KERNEL_TIMES launch of each wavefront form (the shade /
           shadow / closest / sort split); the tol-0.05 adaptive run (min 8,
           step 8, max 64, floor 0.01) with aa=True through both paths
  parent   `python bench.py --gpus 1` on this tree and on the parent commit's
           (DIR: a built checkout of it) in alternating child processes,
           --rounds each: is this tree's K2 line inside the parent's own
           run-to-run spread?  (its own document, --out)
A variant library (PT_HIP_LIB with PT_ALLOW_FOREIGN_BUILD=1) is measured the
same way and named by its own build id."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W = H = 512
SPP, BOUNCES, SEED = 64, 4, 9


def stat(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def edge_mask(obj):
    """Pixels whose 3x3 neighbourhood of first-hit objects is not constant."""
    p = np.pad(obj, 1, mode="edge")
    h, w = obj.shape
    m = np.zeros(obj.shape, dtype=bool)
    for dy in range(3):
        for dx in range(3):
            m |= p[dy:dy + h, dx:dx + w] != obj
    return m


def rmse(a, b, mask):
    return float(np.sqrt(np.mean((a[mask] - b[mask]) ** 2))) if mask.any() else None


def part_parent(args):
    def line(root):
        out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps",
                              str(args.steps), "--warmup", str(args.warmup), "--no-cpu-baseline", "--no-check",
                              "--no-secondary"], cwd=root,
                             capture_output=True, text=True, timeout=600)
        if out.returncode != 0:
            raise SystemExit(f"bench.py in {root} failed:\n{out.stderr[-2000:]}")
        return json.loads(out.stdout.strip().splitlines()[-1])
    rows = {"parent": [], "new": []}
    ids = {}
    for _ in range(args.rounds):
        for name, root in (("parent", os.path.abspath(args.parent_root)), ("new", ROOT)):
            d = line(root)
            rows[name].append(d)
            ids[name] = d.get("build_id")
    def value(d):
        for k in ("ms_per_step", "median_ms", "kernel_ms", "value"):
            if k in d and isinstance(d[k], (int, float)):
                return k, float(d[k])
        raise SystemExit(f"no time in the bench line: {sorted(d)}")
    key = value(rows["new"][0])[0]
    res = {"command": f"bench.py --gpus 1 --steps {args.steps} --warmup {args.warmup} --no-cpu-baseline "
                      "--no-check --no-secondary", "metric": key,
           "rounds": args.rounds}
    for name in rows:
        res[name] = {"build_id": ids[name], key: stat([value(d)[1] for d in rows[name]]),
                     "values": [value(d)[1] for d in rows[name]]}
    res["new_median_inside_parent_spread"] = bool(
        res["parent"][key]["min"] <= res["new"][key]["median"] <= res["parent"][key]["max"])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="uniform,list,effect,bvh")
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--keep", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5, help="part parent: child processes per tree")
    ap.add_argument("--steps", type=int, default=20, help="part parent: bench.py --steps")
    ap.add_argument("--warmup", type=int, default=5, help="part parent: bench.py --warmup")
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    parts = args.parts.split(",")
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "aa_k5.json" if parts == ["k5"] else "aa_k2.json")
    if parts == ["parent"]:
        if not args.parent_root:
            raise SystemExit("--parts parent needs --parent-root")
        res = part_parent(args)
    else:
        res = measure(args, parts)
    text = json.dumps(res, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)


def measure(args, parts):
    import torch
    torch.cuda.set_device(0)
    from pathtracerpython_amd import _native, scene_reader
    from pathtracerpython_amd._abi import make_adapt
    from pathtracerpython_amd.adaptive import Accumulator
    from pathtracerpython_amd.render import Renderer
    scene_reader.VERBOSE = False
    sc = scene_reader.Scene(os.path.join(ROOT, "scenes", "cornell", "cornellroom.sdl"))
    res = {"shape": {"width": W, "height": H, "spp": SPP, "bounces": BOUNCES, "seed": SEED},
           "build_id": _native.build_id(), "library": os.path.relpath(_native.LIB_PATH, ROOT),
           "device": torch.cuda.get_device_name(0), "launches": args.launches, "keep": args.keep}
    npix = W * H

    def last(xs):
        return stat(xs[-args.keep:])

    with Renderer(sc) as r:
        if "uniform" in parts:
            fb = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
            p = {"k_render": r.params(W, H, SPP, BOUNCES, SEED),
                 "k_render_aa": r.params(W, H, SPP, BOUNCES, SEED, aa=True)}
            ms = {k: [] for k in p}
            for _ in range(args.launches):
                for k in p:
                    r.render_device(p[k], fb.data_ptr(), 0)
                    torch.cuda.synchronize()
                    ms[k].append(r.last_kernel_ms())
            u = {k: {"kernel_ms": last(ms[k]),
                     "msamples_per_s": npix * SPP / last(ms[k])["median"] / 1e3} for k in p}
            u["ratio_aa_to_k_render"] = u["k_render_aa"]["kernel_ms"]["median"] / u["k_render"]["kernel_ms"]["median"]
            res["uniform"] = u
        if "list" in parts:
            with Accumulator(r, W, H) as acc:
                p = {"list": r.params(W, H, SPP, BOUNCES, SEED),
                     "list_aa": r.params(W, H, SPP, BOUNCES, SEED, aa=True)}

                def run(k, adapt):
                    """(summed pass kernel ms, wall ms of reset + selects + passes, passes)"""
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    acc.reset()
                    kern, passes = 0.0, []
                    while True:
                        n_active, add = acc.select(adapt)
                        if not n_active:
                            break
                        acc.render(p[k], adapt)
                        torch.cuda.synchronize()
                        kern += r.last_kernel_ms()
                        passes.append((int(n_active), int(add)))
                    return kern, (time.perf_counter() - t0) * 1e3, passes

                out = {}
                for tag, adapt in (("all_64_one_pass", make_adapt(0.0, SPP, SPP, SPP)),
                                   ("adaptive_tol_0.05", make_adapt(0.05, SPP, 8, 8, 0.01))):
                    kern = {k: [] for k in p}
                    wall = {k: [] for k in p}
                    info = {}
                    for _ in range(args.launches):
                        for k in p:
                            a, b, passes = run(k, adapt)
                            kern[k].append(a)
                            wall[k].append(b)
                            info[k] = (passes, acc.read(n=True)["n"])
                    row = {}
                    for k in p:
                        passes, n = info[k]
                        row[k] = {"pass_kernel_ms_sum": last(kern[k]), "wall_ms": last(wall[k]),
                                  "passes": len(passes), "samples": int(n.sum()),
                                  "fraction_of_uniform_budget": float(n.sum()) / (npix * SPP)}
                    row["kernel_ratio_aa_to_list"] = (row["list_aa"]["pass_kernel_ms_sum"]["median"] /
                                                      row["list"]["pass_kernel_ms_sum"]["median"])
                    if tag.startswith("adaptive"):
                        edge = edge_mask(acc.features()["obj"])
                        n0, n1 = info["list"][1].astype(np.int64), info["list_aa"][1].astype(np.int64)
                        row["count_map"] = {
                            "edge_pixels": int(edge.sum()), "other_pixels": int((~edge).sum()),
                            "mean_spp_edge": {"list": float(n0[edge].mean()), "list_aa": float(n1[edge].mean())},
                            "mean_spp_other": {"list": float(n0[~edge].mean()), "list_aa": float(n1[~edge].mean())},
                            "pixels_with_more_samples_under_aa": int((n1 > n0).sum()),
                            "pixels_with_fewer_samples_under_aa": int((n1 < n0).sum()),
                            "edge_pixels_at_min_spp": {"list": int((n0[edge] == 8).sum()),
                                                       "list_aa": int((n1[edge] == 8).sum())}}
                    out[tag] = row
                res["list"] = out
        if "bvh" in parts:
            import tempfile
            from pathtracerpython_amd.synth import write_k5_scene
            Wb = Hb = 512
            k5 = scene_reader.Scene(write_k5_scene(tempfile.mkdtemp(), n_tris=100_000, seed=0, size=Wb))
            with Renderer(k5) as rb:
                fb = torch.empty((Hb, Wb, 3), dtype=torch.float32, device="cuda")
                p = {"wavefront": rb.params(Wb, Hb, 16, BOUNCES, SEED),
                     "single_kernel": rb.params(Wb, Hb, 16, BOUNCES, SEED, megakernel=True),
                     "single_kernel_aa": rb.params(Wb, Hb, 16, BOUNCES, SEED, aa=True, megakernel=True)}
                ms = {k: [] for k in p}
                n = max(4, args.launches // 4)
                for _ in range(n):
                    for k in p:
                        rb.render_device(p[k], fb.data_ptr(), 0)
                        torch.cuda.synchronize()
                        ms[k].append(rb.last_kernel_ms())
                b = {k: {"kernel_ms": stat(ms[k][-max(2, n // 2):])} for k in p}
                b["shape"] = {"scene": "K5 synth", "n_tris": 100_000, "width": Wb, "height": Hb, "spp": 16,
                              "bounces": BOUNCES}
                b["ratio_aa_to_single_kernel"] = (b["single_kernel_aa"]["kernel_ms"]["median"] /
                                                  b["single_kernel"]["kernel_ms"]["median"])
                b["ratio_aa_to_wavefront"] = (b["single_kernel_aa"]["kernel_ms"]["median"] /
                                              b["wavefront"]["kernel_ms"]["median"])
                res["bvh"] = b
        if "k5" in parts:
            res["k5"] = part_k5(args, last)
        if "effect" in parts:
            We = He = 64
            ref = r.render(We, He, 4096, BOUNCES, SEED + 1, out_f64=True, aa=True)
            aa = r.render(We, He, SPP, BOUNCES, SEED, out_f64=True, aa=True)
            centre = r.render(We, He, SPP, BOUNCES, SEED, out_f64=True)
            with Accumulator(r, We, He) as acc:
                edge = edge_mask(acc.features()["obj"])
            res["effect"] = {"width": We, "height": He, "spp": SPP, "reference": "4096 spp antialiased, seed 10",
                             "edge_pixels": int(edge.sum()), "other_pixels": int((~edge).sum()),
                             "rmse_edge": {"aa": rmse(aa, ref, edge), "centre_ray": rmse(centre, ref, edge)},
                             "rmse_other": {"aa": rmse(aa, ref, ~edge), "centre_ray": rmse(centre, ref, ~edge)}}
    return res


def part_k5(args, last):
    """Antialiasing on a BVH scene: the wavefront form of the per-sample
    primary query beside the single kernel and the centre-ray wavefront."""
    import tempfile
    import torch
    from pathtracerpython_amd import scene_reader
    from pathtracerpython_amd._abi import make_adapt
    from pathtracerpython_amd.adaptive import Accumulator
    from pathtracerpython_amd.render import Renderer
    from pathtracerpython_amd.synth import write_k5_scene
    Wb = Hb = 512
    spp = 16
    k5 = scene_reader.Scene(write_k5_scene(tempfile.mkdtemp(), n_tris=100_000, seed=0, size=Wb))
    out = {"shape": {"scene": "K5 synth", "n_tris": 100_000, "width": Wb, "height": Hb, "spp": spp,
                     "bounces": BOUNCES, "seed": SEED}}
    with Renderer(k5) as rb:
        fb = torch.empty((Hb, Wb, 3), dtype=torch.float32, device="cuda")
        p = {"aa_wavefront": rb.params(Wb, Hb, spp, BOUNCES, SEED, aa=True),
             "aa_single_kernel": rb.params(Wb, Hb, spp, BOUNCES, SEED, aa=True, megakernel=True),
             "centre_wavefront": rb.params(Wb, Hb, spp, BOUNCES, SEED)}
        ms = {k: [] for k in p}
        for _ in range(args.launches):
            for k in p:
                rb.render_device(p[k], fb.data_ptr(), 0)
                torch.cuda.synchronize()
                ms[k].append(rb.last_kernel_ms())
        for k in p:
            out[k] = {"kernel_ms": last(ms[k])}
        med = {k: out[k]["kernel_ms"]["median"] for k in p}
        out["ratio_aa_wavefront_to_aa_single_kernel"] = med["aa_wavefront"] / med["aa_single_kernel"]
        out["ratio_aa_wavefront_to_centre_wavefront"] = med["aa_wavefront"] / med["centre_wavefront"]
        out["step_count_floor_of_that_ratio"] = (BOUNCES + 1) / BOUNCES
        # the per-kernel split (the walks one after the other on one stream)
        split = {}
        for k, aa in (("aa_wavefront", True), ("centre_wavefront", False)):
            _, st = rb.render_params(rb.params(Wb, Hb, spp, BOUNCES, SEED, aa=aa, kernel_times=True), stats=True)
            split[k] = {f: st[f] for f in ("shade_ms", "shadow_ms", "closest_ms", "sort_ms", "shade_launches",
                                           "shadow_launches", "closest_launches", "sort_launches")}
        out["kernel_times"] = split
        # the adaptive run, antialiased, through both paths
        with Accumulator(rb, Wb, Hb) as acc:
            adapt = make_adapt(0.05, 64, 8, 8, 0.01)
            pa = {"aa_wavefront": rb.params(Wb, Hb, 64, BOUNCES, SEED, aa=True),
                  "aa_single_kernel": rb.params(Wb, Hb, 64, BOUNCES, SEED, aa=True, megakernel=True)}
            kern = {k: [] for k in pa}
            info = {}
            runs = max(3, args.launches // 5)
            for _ in range(runs):
                for k in pa:
                    acc.reset()
                    t, passes = 0.0, 0
                    while acc.select(adapt)[0]:
                        acc.render(pa[k], adapt)
                        torch.cuda.synchronize()
                        t += rb.last_kernel_ms()
                        passes += 1
                    kern[k].append(t)
                    info[k] = (passes, acc.read(n=True)["n"])
            row = {k: {"pass_kernel_ms_sum": stat(kern[k][-max(2, runs // 2):]), "passes": info[k][0],
                       "samples": int(info[k][1].sum())} for k in pa}
            row["same_count_map"] = bool(np.array_equal(info["aa_wavefront"][1], info["aa_single_kernel"][1]))
            row["kernel_ratio_wavefront_to_single_kernel"] = (
                row["aa_wavefront"]["pass_kernel_ms_sum"]["median"] /
                row["aa_single_kernel"]["pass_kernel_ms_sum"]["median"])
            out["adaptive_tol_0.05"] = row
    return out


if __name__ == "__main__":
    main()
