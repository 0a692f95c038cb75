#!/usr/bin/env python3
"""Measure the adaptive sampler (dev tool; prints one JSON document).

    python3 scripts/bench_adaptive.py [--parts a,b | --parts c] [--reps N] [--out FILE]

The K2 shape: Cornell 512x512, 4 bounces, seed 9, budget 64 samples per pixel.
  a  throughput of the list kernel: tol 0, min = max = 64 in one pass of 64 and
     in 8 passes of 8, beside k_render (the uniform render of the same frame)
     in interleaved rounds of one process; Mpath-samples/s from kernel time
     (HIP events) and from wall time of the whole run, selects included
  b  adaptive runs at tol 0.05 and 0.02 (min 8, step 8): samples, passes, wall
     time of the whole run, RMSE against a 4096-spp uniform frame of another
     seed, and beside it the RMSE of a uniform render of the same total sample
     count; each also as a relative RMSE in the stop rule's normalisation
  c  BVH scenes, the K5 shape (synth, 100k triangles, 1024x1024, 4 bounces,
     budget 64): the wavefront list form beside the single-kernel list pass
     (megakernel=True) and the uniform wavefront render — (i) one pass of 64,
     (ii) 8 passes of 8, (iii) whole runs at tol 0.05 and 0.02 (min 8, step 8):
     samples, passes, wall time.  Written to its own document (--out).
  d  row bands (--parts d [--parent-root DIR]; its own document): (a) the part-b
     tol-0.05 run on this build and on the parent commit's (DIR: a built copy
     of its package and include/) in alternating child processes of one
     command, --rounds rounds each; (b) MultiRenderer.render_adaptive on [0], [0, 0], [0]*4 (and on all
     GPUs when there are several): wall time of the run and of the merge;
     (c) the export and import kernels on one band of 8 of a 4096 x 4096 frame
Reads none of bench.py's artifacts.  Times are medians over --reps rounds
after --warmup rounds, with min and max."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W = H = 512
BOUNCES, SEED, BUDGET = 4, 9, 64


def stat(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def rel_rmse(x, ref, floor=0.01):
    """RMS over pixels of |x - ref|_2 / (|r| + |g| + |b| + floor) of ref: the
    error in the stop rule's own normalisation."""
    e = np.sqrt(((x - ref) ** 2).sum(axis=-1)) / (np.abs(ref).sum(axis=-1) + floor)
    return float(np.sqrt(np.mean(e ** 2)))


def part_c(args):
    """The K5 shape: both list paths and the uniform wavefront render in
    interleaved rounds of one process."""
    import tempfile

    import torch
    from pathtracerpython_amd import _native, scene_reader
    from pathtracerpython_amd._abi import make_adapt
    from pathtracerpython_amd.adaptive import Accumulator, run_passes
    from pathtracerpython_amd.render import Renderer
    from pathtracerpython_amd.synth import write_k5_scene
    scene_reader.VERBOSE = False
    Wc = Hc = 1024
    n_tris = 100_000
    sc = scene_reader.Scene(write_k5_scene(tempfile.mkdtemp(), n_tris=n_tris, seed=0, size=Wc))
    npix = Wc * Hc
    res = {"shape": {"scene": "K5 synth", "n_tris": n_tris, "width": Wc, "height": Hc, "bounces": BOUNCES,
                     "seed": SEED, "budget": BUDGET},
           "build_id": _native.build_id(), "device": torch.cuda.get_device_name(0),
           "reps": args.reps, "warmup": args.warmup}
    with Renderer(sc) as r, Accumulator(r, Wc, Hc) as acc:
        params = {"wavefront": r.params(Wc, Hc, BUDGET, BOUNCES, SEED),
                  "single_kernel": r.params(Wc, Hc, BUDGET, BOUNCES, SEED, megakernel=True)}
        fb = torch.empty((Hc, Wc, 3), dtype=torch.float32, device="cuda")

        def uniform():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r.render_device(params["wavefront"], fb.data_ptr(), 0)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3, r.last_kernel_ms()

        def adaptive(path, adapt):
            """(wall ms of reset + every select and pass, summed pass kernel ms, passes)"""
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            acc.reset()
            passes = run_passes(acc, params[path], adapt)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3, passes

        def pass_kernel_ms(path, adapt):
            acc.reset()
            out = []
            while acc.select(adapt)[0]:
                acc.render(params[path], adapt)
                out.append(r.last_kernel_ms())
            return out

        one = make_adapt(0.0, BUDGET, BUDGET, BUDGET)
        eight = make_adapt(0.0, BUDGET, BUDGET, 8)
        legs = [("uniform_wavefront", None, None)] + \
               [("%s_%s" % (path, tag), path, adapt) for tag, adapt in (("1x64", one), ("8x8", eight))
                for path in ("wavefront", "single_kernel")]
        wall = {name: [] for name, _, _ in legs}
        kern = {name: [] for name, _, _ in legs}
        for i in range(args.warmup + args.reps):
            for name, path, adapt in legs:
                if path is None:
                    w, k = uniform()
                else:
                    w, _ = adaptive(path, adapt)
                    k = sum(pass_kernel_ms(path, adapt))
                if i >= args.warmup:
                    wall[name].append(w)
                    kern[name].append(k)
        t = {}
        for name in wall:
            t[name] = {"wall_ms": stat(wall[name]), "kernel_ms": stat(kern[name]),
                       "msamples_per_s_kernel": npix * BUDGET / statistics.median(kern[name]) / 1e3,
                       "msamples_per_s_wall": npix * BUDGET / statistics.median(wall[name]) / 1e3}
        for name in wall:
            for base in ("uniform_wavefront", "single_kernel_" + name.rsplit("_", 1)[-1]):
                if name != base and base in t:
                    t[name]["kernel_ratio_to_" + base] = (t[name]["kernel_ms"]["median"] /
                                                          t[base]["kernel_ms"]["median"])
                    t[name]["wall_ratio_to_" + base] = (t[name]["wall_ms"]["median"] /
                                                        t[base]["wall_ms"]["median"])
        res["throughput"] = t
        runs = []
        for tol in (0.05, 0.02):
            adapt = make_adapt(tol, BUDGET, 8, 8, 0.01)
            walls = {"wavefront": [], "single_kernel": []}
            got = {}
            for i in range(args.warmup + args.reps):
                for path in walls:
                    w, passes = adaptive(path, adapt)
                    if i >= args.warmup:
                        walls[path].append(w)
                    d = acc.read(n=True)
                    got[path] = (passes, int(d["n"].sum()))
            assert got["wavefront"] == got["single_kernel"]   # the same run on either path
            passes, total = got["wavefront"]
            row = {"tol": tol, "min_spp": 8, "step_spp": 8, "floor": 0.01, "samples": total,
                   "fraction_of_uniform_budget": total / (npix * BUDGET),
                   "passes": [list(x) for x in passes]}
            for path in walls:
                row[path] = {"wall_ms": stat(walls[path]), "pass_kernel_ms": pass_kernel_ms(path, adapt)}
            row["wall_ratio_wavefront_to_single_kernel"] = (row["wavefront"]["wall_ms"]["median"] /
                                                            row["single_kernel"]["wall_ms"]["median"])
            row["wall_ratio_wavefront_to_uniform_budget"] = (row["wavefront"]["wall_ms"]["median"] /
                                                             t["uniform_wavefront"]["wall_ms"]["median"])
            runs.append(row)
        res["adaptive"] = runs
    return res


def cornell_scene():
    from pathtracerpython_amd import scene_reader
    scene_reader.VERBOSE = False
    return scene_reader.Scene(os.path.join(ROOT, "scenes", "cornell", "cornellroom.sdl"))


def part_d_child(args):
    """One process of part d (a): the tol-0.05 K2 run, wall ms of each rep."""
    import torch
    from pathtracerpython_amd import _native
    from pathtracerpython_amd._abi import make_adapt
    from pathtracerpython_amd.adaptive import Accumulator, run_passes
    from pathtracerpython_amd.render import Renderer
    adapt = make_adapt(0.05, BUDGET, 8, 8, 0.01)
    walls = []
    with Renderer(cornell_scene()) as r, Accumulator(r, W, H) as acc:
        p = r.params(W, H, BUDGET, BOUNCES, SEED)
        for i in range(args.warmup + args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            acc.reset()
            passes = run_passes(acc, p, adapt)
            torch.cuda.synchronize()
            if i >= args.warmup:
                walls.append((time.perf_counter() - t0) * 1e3)
        total = int(acc.read(n=True)["n"].sum())
    return {"build_id": _native.build_id(), "wall_ms": walls, "samples": total, "passes": len(passes)}


def part_d(args):
    import subprocess

    import torch
    from pathtracerpython_amd import _native
    from pathtracerpython_amd._abi import make_band
    from pathtracerpython_amd.adaptive import Accumulator, tile_bytes
    from pathtracerpython_amd.render import MultiRenderer, Renderer
    res = {"shape": {"width": W, "height": H, "bounces": BOUNCES, "seed": SEED, "budget": BUDGET,
                     "tol": 0.05, "min_spp": 8, "step_spp": 8},
           "build_id": _native.build_id(), "device": torch.cuda.get_device_name(0),
           "gpus": torch.cuda.device_count()}
    # (a) this build beside the parent's, alternating child processes
    if args.parent_root:
        def child(root):
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--parts", "d_child", "--reps", "3",
                                  "--warmup", "2"] + (["--root", root] if root else []),
                                 capture_output=True, text=True, timeout=120)
            if out.returncode != 0:
                raise SystemExit(f"part d child ({root or 'this build'}) failed:\n{out.stderr[-2000:]}")
            return json.loads(out.stdout.strip().splitlines()[-1])
        rows = {"parent": [], "new": []}
        ids = {}
        for _ in range(args.rounds):
            for name, root in (("parent", os.path.abspath(args.parent_root)), ("new", None)):
                c = child(root)
                ids[name] = (c["build_id"], c["samples"], c["passes"])
                rows[name].append(statistics.median(c["wall_ms"]))
        a = {name: {"build_id": ids[name][0], "samples": ids[name][1], "passes": ids[name][2],
                    "round_median_wall_ms": stat(rows[name])} for name in rows}
        a["new_median_inside_parent_spread"] = bool(
            a["parent"]["round_median_wall_ms"]["min"] <= a["new"]["round_median_wall_ms"]["median"]
            <= a["parent"]["round_median_wall_ms"]["max"])
        res["one_accumulator_vs_parent"] = a
    else:
        res["one_accumulator_vs_parent"] = "not measured: no --parent-root"
    # (b) bands on one GPU serialise: the price of the extra selects and the merge, no scaling
    sc = cornell_scene()
    kw = dict(max_spp=BUDGET, bounces=BOUNCES, seed=SEED, tol=0.05, min_spp=8, step_spp=8)
    sets = [[0], [0, 0], [0] * 4]
    if torch.cuda.device_count() > 1:
        sets.append(list(range(torch.cuda.device_count())))
    b = []
    for ids_ in sets:
        with MultiRenderer(sc, ids_) as m:
            walls, merges, passes = [], [], []
            for i in range(args.warmup + args.reps):
                t = {}
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                r_ = m.render_adaptive(W, H, timings=t, **kw)
                wall = (time.perf_counter() - t0) * 1e3
                if i >= args.warmup:
                    walls.append(wall)
                    merges.append(t["merge_ms"])
                    passes.append(t["passes_ms"])
        b.append({"devices": ids_, "wall_ms": stat(walls), "passes_ms": stat(passes), "merge_ms": stat(merges),
                  "samples": r_.samples, "n_passes": len(r_.passes)})
    res["bands"] = b
    if torch.cuda.device_count() <= 1:
        res["n_gpu_scaling"] = "N-GPU scaling not measured"
    # (c) the tile kernels: 4096^2, one band of 8
    Wc = Hc = 4096
    band = make_band(Hc, 0, Hc, 8, 0)
    nbytes = tile_bytes(Wc, Hc // 8)
    with Renderer(sc) as r, Accumulator(r, Wc, Hc, band=band) as acc:
        tile = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
        s = torch.cuda.current_stream().cuda_stream
        ms = {"export": [], "import": []}
        for i in range(args.warmup + args.reps):
            for name, fn in (("export", lambda: acc.export_band_device(tile.data_ptr(), s)),
                             ("import", lambda: acc.import_band(band, tile.data_ptr(), s))):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                if i >= args.warmup:
                    ms[name].append(e0.elapsed_time(e1))
    peak = 6.29e12   # the measured copy rate of the device, bytes/s
    res["tile_kernels"] = {"width": Wc, "height": Hc, "band": [0, Hc, 8, 0], "pixels": Wc * Hc // 8,
                           "tile_bytes": nbytes}
    for name in ms:
        med = statistics.median(ms[name])
        res["tile_kernels"][name] = {"ms": stat(ms[name]), "bytes_moved": 2 * nbytes,
                                     "share_of_copy_rate": 2 * nbytes / (med * 1e-3) / peak}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="a,b")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=10, help="part d (a): child processes per build")
    ap.add_argument("--parent-root", default=None,
                    help="part d (a): a directory with the parent commit's built package and include/")
    ap.add_argument("--root", default=None, help="(part d's children) import the package from here")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.root:
        sys.path.insert(0, os.path.abspath(args.root))
    import torch
    torch.cuda.set_device(0)
    if args.parts == "d_child":
        print(json.dumps(part_d_child(args)))
        return
    if args.parts in ("c", "d"):   # documents of their own
        text = json.dumps((part_c if args.parts == "c" else part_d)(args), indent=1)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(text + "\n")
        print(text)
        return
    from pathtracerpython_amd import _native, scene_reader
    from pathtracerpython_amd._abi import make_adapt
    from pathtracerpython_amd.adaptive import Accumulator, run_passes
    from pathtracerpython_amd.render import Renderer
    scene_reader.VERBOSE = False
    sc = scene_reader.Scene(os.path.join(ROOT, "scenes", "cornell", "cornellroom.sdl"))
    torch.cuda.set_device(0)
    res = {"shape": {"width": W, "height": H, "bounces": BOUNCES, "seed": SEED, "budget": BUDGET},
           "build_id": _native.build_id(), "device": torch.cuda.get_device_name(0),
           "reps": args.reps, "warmup": args.warmup}
    parts = args.parts.split(",")
    npix = W * H
    with Renderer(sc) as r, Accumulator(r, W, H) as acc:
        p = r.params(W, H, BUDGET, BOUNCES, SEED)
        fb = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")

        def uniform():
            t0 = time.perf_counter()
            r.render_device(p, fb.data_ptr(), 0)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3, r.last_kernel_ms()

        def adaptive(adapt):
            """(wall ms of reset + every select and pass, passes)"""
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            acc.reset()
            passes = run_passes(acc, p, adapt)   # (kernel times: pass_kernel_ms, timed apart)
            torch.cuda.synchronize()
            wall = (time.perf_counter() - t0) * 1e3
            return wall, passes

        def pass_kernel_ms(adapt):
            acc.reset()
            out = []
            while acc.select(adapt)[0]:
                acc.render(p, adapt)
                out.append(r.last_kernel_ms())
            return out

        if "a" in parts:
            one = make_adapt(0.0, BUDGET, BUDGET, BUDGET)
            eight = make_adapt(0.0, BUDGET, BUDGET, 8)
            rows = {"k_render": [], "list_1x64": [], "list_8x8": []}
            kern = {"k_render": [], "list_1x64": [], "list_8x8": []}
            for i in range(args.warmup + args.reps):
                w_u, k_u = uniform()
                w_1, _ = adaptive(one)
                k_1 = sum(pass_kernel_ms(one))
                w_8, _ = adaptive(eight)
                k_8 = sum(pass_kernel_ms(eight))
                if i >= args.warmup:
                    for name, w, k in (("k_render", w_u, k_u), ("list_1x64", w_1, k_1),
                                       ("list_8x8", w_8, k_8)):
                        rows[name].append(w)
                        kern[name].append(k)
            a = {}
            for name in rows:
                a[name] = {"wall_ms": stat(rows[name]), "kernel_ms": stat(kern[name]),
                           "msamples_per_s_kernel": npix * BUDGET / statistics.median(kern[name]) / 1e3,
                           "msamples_per_s_wall": npix * BUDGET / statistics.median(rows[name]) / 1e3}
            for name in ("list_1x64", "list_8x8"):
                a[name]["kernel_ratio_to_k_render"] = (a[name]["kernel_ms"]["median"] /
                                                       a["k_render"]["kernel_ms"]["median"])
                a[name]["wall_ratio_to_k_render"] = (a[name]["wall_ms"]["median"] /
                                                     a["k_render"]["wall_ms"]["median"])
            sel = []   # the three select kernels of one pass (HIP events), full frame active
            for _ in range(args.warmup + args.reps):
                acc.reset()
                acc.select(one)
                sel.append(r.last_kernel_ms())
            a["select_kernel_ms"] = stat(sel[args.warmup:])
            res["throughput"] = a
        if "b" in parts:
            # (another seed: the reference shares no sample with the frames it judges)
            ref = r.render(W, H, spp=4096, bounces=BOUNCES, seed=SEED + 1, out_f64=True)
            b = []
            for tol in (0.05, 0.02):
                adapt = make_adapt(tol, BUDGET, 8, 8, 0.01)
                walls = []
                for i in range(args.warmup + args.reps):
                    w, passes = adaptive(adapt)
                    if i >= args.warmup:
                        walls.append(w)
                d = acc.read(S=True, n=True)
                mean = d["S"] / d["n"][..., None]
                total = int(d["n"].sum())
                spp_u = max(1, int(round(total / npix)))
                uni = r.render(W, H, spp=spp_u, bounces=BOUNCES, seed=SEED, out_f64=True)
                b.append({"tol": tol, "min_spp": 8, "step_spp": 8, "floor": 0.01,
                          "samples": total, "fraction_of_uniform_budget": total / (npix * BUDGET),
                          "passes": [list(x) for x in passes], "wall_ms": stat(walls),
                          "pass_kernel_ms": pass_kernel_ms(adapt),
                          "rmse_vs_4096spp": float(np.sqrt(np.mean((mean - ref) ** 2))),
                          "rel_rmse_vs_4096spp": rel_rmse(mean, ref),
                          "uniform_same_samples": {
                              "spp": spp_u, "samples": spp_u * npix,
                              "rmse_vs_4096spp": float(np.sqrt(np.mean((uni - ref) ** 2))),
                              "rel_rmse_vs_4096spp": rel_rmse(uni, ref)},
                          "uniform_budget_rmse_vs_4096spp": None})
            full = r.render(W, H, spp=BUDGET, bounces=BOUNCES, seed=SEED, out_f64=True)
            for x in b:
                x["uniform_budget_rmse_vs_4096spp"] = float(np.sqrt(np.mean((full - ref) ** 2)))
            res["adaptive"] = b
    text = json.dumps(res, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
