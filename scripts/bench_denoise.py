#!/usr/bin/env python3
"""Measure the denoiser (dev tool; prints one JSON document per frame shape).

    python3 scripts/bench_denoise.py --shape k2 [--reps N] [--warmup N] [--out FILE]
    python3 scripts/bench_denoise.py --shape k4 ...

Shapes: k2 = Cornell 512x512 (the K2 frame), k4 = Cornell 4096x4096 (the K4
frame shape), 4 bounces, seed 9.  The accumulator is filled by an adaptive run
(k2: tol 0.05, budget 64, min 8, step 8 — the run of profiles/adaptive_k2.json;
k4: the same rule with budget 16), then
  launches   HIP-event time of every launch of pt_accum_denoise_device
             (pt_denoise_times: k_accum_moments, each k_denoise_iter, the
             store), medians over --reps calls after --warmup, and of
             k_features on a fresh accumulator
  call       the whole call (moments + iterations + store) between the scene
             handle's events, timing off
  model      148 B per pixel and iteration (c and v read and written at 48 B
             each, obj, N and P at 52 B) over each iteration's time, as a
             fraction of the 6.29 TB/s copy rate
  adaptive   (k2) the tol-0.05 adaptive run re-measured in this process (wall
             time of reset + selects + passes), the denoise call as a share
             of it
  quality    (k2) tol 0.05 and 0.02: RMSE and relative RMSE of the noisy and
             of the filtered frame against a 4096-spp frame of another seed
Reads none of bench.py's artifacts."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BOUNCES, SEED = 4, 9
BYTES_PER_PIXEL_ITER = 148
COPY_RATE = 6.29e12   # B/s, the measured device copy rate


def stat(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def rel_rmse(x, ref, floor=0.01):
    e = np.sqrt(((x - ref) ** 2).sum(axis=-1)) / (np.abs(ref).sum(axis=-1) + floor)
    return float(np.sqrt(np.mean(e ** 2)))


def rmse(x, ref):
    return float(np.sqrt(np.mean((x - ref) ** 2)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=("k2", "k4"), default="k2")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    torch.cuda.set_device(0)
    from pathtracerpython_amd import _native, scene_reader
    from pathtracerpython_amd._abi import make_adapt
    from pathtracerpython_amd.adaptive import Accumulator, run_passes
    from pathtracerpython_amd.render import Renderer
    scene_reader.VERBOSE = False
    sc = scene_reader.Scene(os.path.join(ROOT, "scenes", "cornell", "cornellroom.sdl"))
    W = H = 512 if args.shape == "k2" else 4096
    budget = 64 if args.shape == "k2" else 16
    npix = W * H
    lib = _native.lib()
    res = {"shape": {"name": args.shape, "width": W, "height": H, "bounces": BOUNCES, "seed": SEED,
                     "budget": budget, "iters": args.iters},
           "build_id": _native.build_id(), "device": torch.cuda.get_device_name(0),
           "reps": args.reps, "warmup": args.warmup}

    def times():
        buf = (C.c_float * 16)()
        n = C.c_int32(0)
        _native.check(lib.pt_denoise_times(1, buf, 16, C.byref(n)), "pt_denoise_times")
        return [float(buf[i]) for i in range(n.value)]

    with Renderer(sc) as r:
        p = r.params(W, H, budget, BOUNCES, SEED)
        adapt = make_adapt(0.05, budget, 8, 8, 0.01)
        out = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
        var = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
        s = torch.cuda.current_stream().cuda_stream
        # k_features: a fresh accumulator each time (the features are kept)
        feat = []
        for i in range(min(args.reps, 8) + 2):
            with Accumulator(r, W, H) as a0:
                _native.check(lib.pt_accum_features(a0._h, C.c_void_p(s)), "pt_accum_features")
                torch.cuda.synchronize()
                if i >= 2:
                    feat.append(r.last_kernel_ms())
        with Accumulator(r, W, H) as acc:
            passes = run_passes(acc, p, adapt)
            d = acc.read(n=True)
            res["fill"] = {"tol": 0.05, "passes": len(passes), "samples": int(d["n"].sum()),
                           "mean_spp": float(d["n"].mean())}
            # per-launch times
            lib.pt_denoise_times(1, None, 0, None)
            rows = []
            for i in range(args.warmup + args.reps):
                acc.denoise_device(out.data_ptr(), var.data_ptr(), False, s, iters=args.iters)
                if i >= args.warmup:
                    rows.append(times())
            lib.pt_denoise_times(0, None, 0, None)
            assert all(len(x) == args.iters + 2 for x in rows)
            cols = list(zip(*rows))
            launches = {"k_features_ms": stat(feat), "k_accum_moments_ms": stat(cols[0]),
                        "k_denoise_store_f32_ms": stat(cols[-1])}
            model = []
            for i in range(args.iters):
                t = stat(cols[1 + i])
                launches["k_denoise_iter_stride%d_ms" % (1 << i)] = t
                rate = npix * BYTES_PER_PIXEL_ITER / (t["median"] * 1e-3)
                model.append({"stride": 1 << i, "ms": t["median"], "model_bytes": npix * BYTES_PER_PIXEL_ITER,
                              "model_TB_per_s": rate / 1e12, "fraction_of_copy_rate": rate / COPY_RATE})
            launches["sum_of_launches_ms"] = stat([sum(x) for x in rows])
            res["launches"] = launches
            res["model"] = {"bytes_per_pixel_iteration": BYTES_PER_PIXEL_ITER, "copy_rate_TB_per_s": COPY_RATE / 1e12,
                            "iterations": model}
            # the whole call, timing off
            call = []
            for i in range(args.warmup + args.reps):
                acc.denoise_device(out.data_ptr(), var.data_ptr(), False, s, iters=args.iters)
                torch.cuda.synchronize()
                if i >= args.warmup:
                    call.append(r.last_kernel_ms())
            res["call_ms"] = stat(call)
            if args.shape == "k2":
                walls = []
                for i in range(args.warmup + args.reps):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    acc.reset()
                    run_passes(acc, p, adapt)
                    torch.cuda.synchronize()
                    if i >= args.warmup:
                        walls.append((time.perf_counter() - t0) * 1e3)
                res["adaptive_tol_0.05"] = {"wall_ms": stat(walls),
                                            "denoise_call_share": res["call_ms"]["median"] / statistics.median(walls),
                                            "features_share": statistics.median(feat) / statistics.median(walls)}
                ref = r.render(W, H, spp=4096, bounces=BOUNCES, seed=SEED + 1, out_f64=True)
                q = []
                for tol in (0.05, 0.02):
                    acc.reset()
                    run_passes(acc, p, make_adapt(tol, budget, 8, 8, 0.01))
                    dd = acc.read(S=True, n=True)
                    noisy = dd["S"] / dd["n"][..., None]
                    filt, _ = acc.denoise(iters=args.iters)
                    q.append({"tol": tol, "samples": int(dd["n"].sum()),
                              "rmse_noisy": rmse(noisy, ref), "rmse_filtered": rmse(filt, ref),
                              "rel_rmse_noisy": rel_rmse(noisy, ref), "rel_rmse_filtered": rel_rmse(filt, ref),
                              "rmse_ratio": rmse(filt, ref) / rmse(noisy, ref)})
                res["quality_vs_4096spp"] = q
    text = json.dumps(res, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
