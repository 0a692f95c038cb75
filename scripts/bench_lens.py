#!/usr/bin/env python3
"""Measure the thin-lens camera (PT_FLAG_LENS; dev tool; prints one JSON
document and writes it to --out, default profiles/lens_k2.json, stamped with
pt_build_id).

    python3 scripts/bench_lens.py [--parts uniform,list,effect] [--out FILE]
    python3 scripts/bench_lens.py --parts parent --parent-root DIR [--rounds 5]

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
           default profiles/lens_k2_parent.json)"""
import argparse
import json
import os
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
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    parts = args.parts.split(",")
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "lens_k2_parent.json" if parts == ["parent"] else "lens_k2.json")
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
