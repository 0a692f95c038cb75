#!/usr/bin/env python3
"""The host side of a launch in this tree beside another build's (dev tool: a
change to pt_plan.h or to pt_hip.hip's entry points that leaves the device code
alone, so only host time could move).

    python3 scripts/bench_host_plan.py --other-lib PATH/libpt_hip.so [--rounds 5] [--out FILE]

Alternating child processes on one card, --rounds per library: this tree's
own, and the other one loaded with PT_HIP_LIB and PT_ALLOW_FOREIGN_BUILD=1
(e.g. the parent commit's, built in a checkout of it).  Each round measures
  k2, k5     `bench.py --config k2 / k5` ms per step
  small      pt_render_device of 64x64, 16 spp, 4 bounces on the K5 synth scene
             (the wavefront kernels: 6 steps of a few launches each), --launches
             calls back to back on one stream: host microseconds per call until
             the call returns (enqueue_us) and until the stream is idle
             (wall_us), per process the median of 5 such batches after a warm-up.
Writes per number both libraries' values, their median / min / max, and
whether this tree's median lies inside the other's own min-max (default
profiles/refactor_plan.json).  A child that fails ends the run."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
W = H = 64
SPP, BOUNCES, SEED = 16, 4, 9
NUMBERS = ("k2_ms_per_step", "k5_ms_per_step", "small_enqueue_us", "small_wall_us")


def child(launches):
    import tempfile
    import torch
    torch.cuda.set_device(0)
    from pathtracerpython_amd import _native, scene_reader
    from pathtracerpython_amd._abi import PT_PATH_WAVEFRONT
    from pathtracerpython_amd.render import Renderer
    from pathtracerpython_amd.synth import write_k5_scene
    scene_reader.VERBOSE = False
    k5 = scene_reader.Scene(write_k5_scene(tempfile.mkdtemp(), n_tris=20_000, seed=0, size=W))
    enq, wall = [], []
    with Renderer(k5) as r:
        p = r.params(W, H, SPP, BOUNCES, SEED)
        out = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
        for batch in range(6):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(launches):
                r.render_device(p, out.data_ptr())
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            if batch:   # (the first batch warms up)
                enq.append((t1 - t0) / launches * 1e6)
                wall.append((t2 - t0) / launches * 1e6)
        assert r.last_launch()["path"] == PT_PATH_WAVEFRONT
    print(json.dumps({"build_id": _native.build_id(), "small_enqueue_us": statistics.median(enq),
                      "small_wall_us": statistics.median(wall)}))


def run(cmd, env, timeout):
    out = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    if out.returncode != 0:
        raise SystemExit(f"{' '.join(cmd)} failed ({out.returncode}):\n{out.stderr[-2000:]}")
    line = out.stdout.strip().splitlines()[-1]
    print(os.path.basename(cmd[1]), env.get("PT_HIP_LIB", "this tree"), line[:200], file=sys.stderr, flush=True)
    return json.loads(line)


def stat(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "values": xs}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--other-lib", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refactor_plan.json"))
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args.launches)
    if not args.other_lib:
        raise SystemExit("--other-lib: the library to compare against")
    envs = {"other": dict(os.environ, PT_HIP_LIB=os.path.abspath(args.other_lib), PT_ALLOW_FOREIGN_BUILD="1"),
            "this": {k: v for k, v in os.environ.items() if k not in ("PT_HIP_LIB", "PT_ALLOW_FOREIGN_BUILD")}}
    bench = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--no-cpu-baseline", "--no-check",
             "--no-secondary", "--config"]
    small = [sys.executable, os.path.abspath(__file__), "--child", "--launches", str(args.launches)]
    rows = {t: {n: [] for n in NUMBERS} for t in envs}
    ids = {}
    for _ in range(args.rounds):
        for t, env in envs.items():
            rows[t]["k2_ms_per_step"].append(run(bench + ["k2"], env, 300)["ms_per_step"])
            rows[t]["k5_ms_per_step"].append(run(bench + ["k5"], env, 600)["ms_per_step"])
            s = run(small, env, 300)
            ids[t] = s["build_id"]   # (bench.py loads the same library: _native.LIB_PATH)
            rows[t]["small_enqueue_us"].append(s["small_enqueue_us"])
            rows[t]["small_wall_us"].append(s["small_wall_us"])
    res = {"shape": {"k2_ms_per_step": "bench.py --gpus 1 --config k2 (its default steps and warm-up)",
                     "k5_ms_per_step": "bench.py --gpus 1 --config k5 (its default steps and warm-up)",
                     "small": {"scene": "K5 synth", "n_tris": 20_000, "width": W, "height": H, "spp": SPP,
                               "bounces": BOUNCES, "seed": SEED, "launches": args.launches}},
           "rounds": args.rounds, "build_id": ids, "numbers": {}}
    for n in NUMBERS:
        o, t = stat(rows["other"][n]), stat(rows["this"][n])
        res["numbers"][n] = {"other": o, "this": t,
                             "this_median_inside_other_spread": bool(o["min"] <= t["median"] <= o["max"])}
    text = json.dumps(res, indent=1)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
