#!/usr/bin/env python3
"""Measure the thin-lens camera (PT_FLAG_LENS; dev tool; prints one JSON
document and writes it to --out, default profiles/lens_k2.json, stamped with
pt_build_id).

    python3 scripts/bench_lens.py [--parts uniform,list,effect] [--out FILE]
    python3 scripts/bench_lens.py --parts k5            (writes profiles/lens_k5.json)
    python3 scripts/bench_lens.py --parts parent --parent-root DIR [--rounds 5]
    python3 scripts/bench_lens.py --parts parent_k5 --parent-root DIR [--rounds 5]

The K2 frame: Cornell 512x512, 64 spp, 4 bounces, seed 9, lens R = 0.25,
zf = -24.  Kernel times are HIP events (pt_last_kernel_ms), one process, the
legs alternating, --launches launches each (default 20), the median of the
last --keep (default 10).
  uniform  k_render, k_render_aa and k_render_lens with and without PT_FLAG_AA
           on one lens scene (the first two with lens=False: the pinhole
           kernels on the lens scene's records); the yardstick is k_render_aa
  list     k_render_list_lens beside k_render_list_aa (both antialiased): all
           64 samples in one pass, and the tol-0.05 adaptive run (min 8, step
           8, floor 0.01): summed pass kernel time, samples, passes
  effect   Cornell 64x64, 64 spp: RMSE of a lens frame and of a pinhole frame
           (both antialiased) against a 4096-spp lens frame of another seed
  parent   `python bench.py --gpus 1` on this tree and on the parent commit's
           (DIR: a built checkout of it) in alternating child processes,
           --rounds each (scripts/bench_aa.py part_parent; its own document,
           default profiles/lens_k2_parent.json)
  k5       a scene with a BVH (synth.write_k5_scene, 100k triangles, seed 0,
           512x512, 16 spp, 4 bounces, the same lens): the lens through the
           wavefront kernels (pt_shade_lens.hip) with and without PT_FLAG_AA
           beside the lens single kernel (megakernel=True), the antialiased and
           the centre-ray wavefront render (lens=False), each launch's path
           from pt_last_launch_info; and all 64 samples in one list pass
           through both lens paths
  parent_k5  `python bench.py --gpus 1` and `python bench.py --gpus 1 --config
           k5` (bench.py's own steps and warm-up) on this tree and on the
           parent commit's, alternating child processes, --rounds each: the
           parent's min-max and this tree's median per config (its own
           document, default profiles/lens_k5_parent.json)"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from bench_aa import part_parent, stat  # noqa: E402

W = H = 512
SPP, BOUNCES, SEED = 64, 4, 9
LENS = (0.25, -24.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="uniform,list,effect")
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--keep", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5, help="part parent: child processes per tree")
    ap.add_argument("--steps", type=int, default=20, help="part parent: bench.py --steps")
    ap.add_argument("--warmup", type=int, default=5, help="part parent: bench.py --warmup")
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--configs", default="k2,k5", help="part parent_k5: bench.py --config values")
    ap.add_argument("--order", default="parent,new", help="part parent_k5: which tree runs first in a round")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    parts = args.parts.split(",")
    if args.out is None:
        name = {"parent": "lens_k2_parent.json", "parent_k5": "lens_k5_parent.json", "k5": "lens_k5.json"}
        args.out = os.path.join(ROOT, "profiles", name.get(parts[0], "lens_k2.json") if len(parts) == 1
                                else "lens_k2.json")
    if parts in (["parent"], ["parent_k5"]):
        if not args.parent_root:
            raise SystemExit("--parts %s needs --parent-root" % parts[0])
        res = part_parent(args) if parts == ["parent"] else part_parent_k5(args)
    elif parts == ["k5"]:
        res = part_k5(args)
    else:
        res = measure(args, parts)
    text = json.dumps(res, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)


def part_parent_k5(args):
    """bench.py's K2 and K5 lines of the parent's tree and of this one, in
    alternating child processes."""
    def line(root, config):
        out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--config", config],
                             cwd=root, capture_output=True, text=True, timeout=900)
        if out.returncode != 0:
            raise SystemExit(f"bench.py --config {config} in {root} failed:\n{out.stderr[-2000:]}")
        d = json.loads(out.stdout.strip().splitlines()[-1])
        print(f"{config} {os.path.relpath(root, ROOT)}: {d['ms_per_step']:.4f} ms per step", file=sys.stderr, flush=True)
        return d
    roots = {"parent": os.path.abspath(args.parent_root), "new": ROOT}
    trees = tuple((name, roots[name]) for name in args.order.split(","))
    res = {"rounds": args.rounds, "order": ", ".join(n for n, _ in trees) + ", ... per config"}
    for config in args.configs.split(","):
        rows = {name: [] for name, _ in trees}
        for _ in range(args.rounds):
            for name, root in trees:
                rows[name].append(line(root, config))
        row = {"command": "bench.py --gpus 1 --config " + config, "metric": "ms_per_step"}
        for name in rows:
            v = [float(d["ms_per_step"]) for d in rows[name]]
            row[name] = {"build_id": rows[name][-1].get("build_id"), "ms_per_step": stat(v), "values": v,
                         "value": stat([float(d["value"]) for d in rows[name]]), "unit": rows[name][-1].get("unit")}
        row["new_median_inside_parent_spread"] = bool(
            row["parent"]["ms_per_step"]["min"] <= row["new"]["ms_per_step"]["median"]
            <= row["parent"]["ms_per_step"]["max"])
        res[config] = row
    return res


def part_k5(args):
    """The lens on a BVH scene: its wavefront form beside the single kernel,
    the antialiased and the centre-ray wavefront render."""
    import tempfile
    import torch
    torch.cuda.set_device(0)
    from pathtracerpython_amd import _native, scene_reader
    from pathtracerpython_amd._abi import PATH_NAMES, make_adapt
    from pathtracerpython_amd.adaptive import Accumulator
    from pathtracerpython_amd.render import Renderer
    from pathtracerpython_amd.synth import write_k5_scene
    scene_reader.VERBOSE = False
    Wb = Hb = 512
    spp, bounces = 16, 4
    k5 = scene_reader.Scene(write_k5_scene(tempfile.mkdtemp(), n_tris=100_000, seed=0, size=Wb))
    out = {"shape": {"scene": "K5 synth", "n_tris": 100_000, "width": Wb, "height": Hb, "spp": spp,
                     "bounces": bounces, "seed": SEED, "lens": {"radius": LENS[0], "focus_z": LENS[1]}},
           "build_id": _native.build_id(), "library": os.path.relpath(_native.LIB_PATH, ROOT),
           "device": torch.cuda.get_device_name(0), "launches": args.launches, "keep": args.keep}

    def last(xs):
        return stat(xs[-args.keep:])

    with Renderer(k5, lens=LENS) as rb:
        fb = torch.empty((Hb, Wb, 3), dtype=torch.float32, device="cuda")
        p = {"lens_aa_wavefront": rb.params(Wb, Hb, spp, bounces, SEED, aa=True),
             "lens_wavefront": rb.params(Wb, Hb, spp, bounces, SEED),
             "lens_aa_single_kernel": rb.params(Wb, Hb, spp, bounces, SEED, aa=True, megakernel=True),
             "lens_single_kernel": rb.params(Wb, Hb, spp, bounces, SEED, megakernel=True),
             "aa_wavefront": rb.params(Wb, Hb, spp, bounces, SEED, aa=True, lens=False),
             "centre_wavefront": rb.params(Wb, Hb, spp, bounces, SEED, lens=False)}
        ms = {k: [] for k in p}
        info = {}
        for _ in range(args.launches):
            for k in p:
                rb.render_device(p[k], fb.data_ptr(), 0)
                torch.cuda.synchronize()
                ms[k].append(rb.last_kernel_ms())
                info[k] = rb.last_launch()
        for k in p:
            out[k] = {"kernel_ms": last(ms[k]), "path": PATH_NAMES[info[k]["path"]], "steps": info[k]["steps"],
                      "lanes_per_pixel": info[k]["lanes_per_pixel"]}
        med = {k: out[k]["kernel_ms"]["median"] for k in p}
        out["ratio_lens_aa_wavefront_to_lens_aa_single_kernel"] = med["lens_aa_wavefront"] / med["lens_aa_single_kernel"]
        out["ratio_lens_wavefront_to_lens_single_kernel"] = med["lens_wavefront"] / med["lens_single_kernel"]
        out["ratio_lens_aa_wavefront_to_aa_wavefront"] = med["lens_aa_wavefront"] / med["aa_wavefront"]
        out["ratio_lens_wavefront_to_centre_wavefront"] = med["lens_wavefront"] / med["centre_wavefront"]
        # all 64 samples in one list pass through both lens paths
        with Accumulator(rb, Wb, Hb) as acc:
            adapt = make_adapt(0.0, 64, 64, 64)
            pa = {"lens_aa_wavefront": rb.params(Wb, Hb, 64, bounces, SEED, aa=True),
                  "lens_aa_single_kernel": rb.params(Wb, Hb, 64, bounces, SEED, aa=True, megakernel=True)}
            kern = {k: [] for k in pa}
            linfo, n = {}, {}
            runs = max(3, args.launches // 5)
            for _ in range(runs):
                for k in pa:
                    acc.reset()
                    acc.render(pa[k], adapt)
                    torch.cuda.synchronize()
                    kern[k].append(rb.last_kernel_ms())
                    linfo[k] = rb.last_launch()
                    n[k] = acc.read(S=True, n=True)
            row = {k: {"pass_kernel_ms": stat(kern[k][-max(2, runs // 2):]), "path": PATH_NAMES[linfo[k]["path"]],
                       "steps": linfo[k]["steps"], "lanes_per_pixel": linfo[k]["lanes_per_pixel"],
                       "samples": int(n[k]["n"].sum())} for k in pa}
            row["same_sums_bit_for_bit"] = bool(np.array_equal(n["lens_aa_wavefront"]["S"].view(np.uint64),
                                                               n["lens_aa_single_kernel"]["S"].view(np.uint64)))
            row["kernel_ratio_wavefront_to_single_kernel"] = (
                row["lens_aa_wavefront"]["pass_kernel_ms"]["median"] /
                row["lens_aa_single_kernel"]["pass_kernel_ms"]["median"])
            out["list_all_64_one_pass"] = row
    return out


def measure(args, parts):
    import torch
    torch.cuda.set_device(0)
    from pathtracerpython_amd import _native, scene_reader
    from pathtracerpython_amd._abi import make_adapt
    from pathtracerpython_amd.adaptive import Accumulator
    from pathtracerpython_amd.render import Renderer
    scene_reader.VERBOSE = False
    sc = scene_reader.Scene(os.path.join(ROOT, "scenes", "cornell", "cornellroom.sdl"))
    res = {"shape": {"width": W, "height": H, "spp": SPP, "bounces": BOUNCES, "seed": SEED,
                     "lens": {"radius": LENS[0], "focus_z": LENS[1]}},
           "build_id": _native.build_id(), "library": os.path.relpath(_native.LIB_PATH, ROOT),
           "device": torch.cuda.get_device_name(0), "launches": args.launches, "keep": args.keep}
    npix = W * H

    def last(xs):
        return stat(xs[-args.keep:])

    with Renderer(sc, lens=LENS) as r:
        if "uniform" in parts:
            fb = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
            p = {"k_render": r.params(W, H, SPP, BOUNCES, SEED, lens=False),
                 "k_render_aa": r.params(W, H, SPP, BOUNCES, SEED, aa=True, lens=False),
                 "k_render_lens": r.params(W, H, SPP, BOUNCES, SEED),
                 "k_render_lens_aa": r.params(W, H, SPP, BOUNCES, SEED, aa=True)}
            ms = {k: [] for k in p}
            for _ in range(args.launches):
                for k in p:
                    r.render_device(p[k], fb.data_ptr(), 0)
                    torch.cuda.synchronize()
                    ms[k].append(r.last_kernel_ms())
            u = {k: {"kernel_ms": last(ms[k]),
                     "msamples_per_s": npix * SPP / last(ms[k])["median"] / 1e3} for k in p}
            med = {k: u[k]["kernel_ms"]["median"] for k in p}
            u["ratio_lens_aa_to_k_render_aa"] = med["k_render_lens_aa"] / med["k_render_aa"]
            u["ratio_lens_to_k_render_aa"] = med["k_render_lens"] / med["k_render_aa"]
            u["ratio_lens_aa_to_k_render"] = med["k_render_lens_aa"] / med["k_render"]
            u["extra_ms_lens_aa_over_k_render_aa"] = med["k_render_lens_aa"] - med["k_render_aa"]
            res["uniform"] = u
        if "list" in parts:
            with Accumulator(r, W, H) as acc:
                p = {"list_aa": r.params(W, H, SPP, BOUNCES, SEED, aa=True, lens=False),
                     "list_lens_aa": r.params(W, H, SPP, BOUNCES, SEED, aa=True)}

                def run(k, adapt):
                    acc.reset()
                    kern, passes = 0.0, 0
                    while acc.select(adapt)[0]:
                        acc.render(p[k], adapt)
                        torch.cuda.synchronize()
                        kern += r.last_kernel_ms()
                        passes += 1
                    return kern, passes

                out = {}
                for tag, adapt in (("all_64_one_pass", make_adapt(0.0, SPP, SPP, SPP)),
                                   ("adaptive_tol_0.05", make_adapt(0.05, SPP, 8, 8, 0.01))):
                    kern = {k: [] for k in p}
                    info = {}
                    for _ in range(args.launches):
                        for k in p:
                            a, passes = run(k, adapt)
                            kern[k].append(a)
                            info[k] = (passes, acc.read(n=True)["n"])
                    row = {k: {"pass_kernel_ms_sum": last(kern[k]), "passes": info[k][0],
                               "samples": int(info[k][1].sum()),
                               "fraction_of_uniform_budget": float(info[k][1].sum()) / (npix * SPP)} for k in p}
                    row["kernel_ratio_lens_to_aa"] = (row["list_lens_aa"]["pass_kernel_ms_sum"]["median"] /
                                                      row["list_aa"]["pass_kernel_ms_sum"]["median"])
                    out[tag] = row
                res["list"] = out
        if "effect" in parts:
            We = He = 64
            ref = r.render(We, He, 4096, BOUNCES, SEED + 1, out_f64=True, aa=True)
            lens = r.render(We, He, SPP, BOUNCES, SEED, out_f64=True, aa=True)
            pin = r.render(We, He, SPP, BOUNCES, SEED, out_f64=True, aa=True, lens=False)
            pin_ref = r.render(We, He, 4096, BOUNCES, SEED + 1, out_f64=True, aa=True, lens=False)
            rm = lambda a, b: float(np.sqrt(np.mean((a - b) ** 2)))
            res["effect"] = {"width": We, "height": He, "spp": SPP,
                             "reference": "4096 spp through the lens, antialiased, seed 10",
                             "rmse_lens_64spp": rm(lens, ref), "rmse_pinhole_64spp": rm(pin, ref),
                             "rmse_pinhole_4096spp": rm(pin_ref, ref)}
    return res


if __name__ == "__main__":
    main()
