#!/usr/bin/env python3
"""The wavefront shade kernels of this tree beside another build's (dev tool:
a change to pt_shade.hip / pt_wavefront.h that may move their code).

    python3 scripts/bench_wf_shade.py --other-lib PATH/libpt_hip.so [--rounds 5] [--out FILE]

Alternating child processes on one card, --rounds per library: this tree's
own, and the other one loaded with PT_HIP_LIB and PT_ALLOW_FOREIGN_BUILD=1
(e.g. the parent commit's, built in a checkout of it).  Each round measures
  k5         `bench.py --config k5` ms per step (1024x1024, 256 spp)
  shade_ms   of PT_FLAG_KERNEL_TIMES launches on the K5 synth scene at 512x512,
             16 spp, 4 bounces (the scene of profiles/aa_k5.json), for the four
             shade kernels: the frame and one accumulator pass of 16 samples
             over every pixel, centre rays and antialiased; per process the
             median of --launches launches after one warm-up.
Writes per number both libraries' values, their median / min / max, and
whether this tree's median lies inside the other's own min-max (default
profiles/refactor_wf_shade.json).  A child that fails ends the run."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
W = H = 512
SPP, BOUNCES, SEED = 16, 4, 9
FORMS = ("k_wf_shade", "k_wf_shade_aa", "k_wf_shade_list", "k_wf_shade_list_aa")


def child(launches):
    import tempfile
    import torch
    torch.cuda.set_device(0)
    from pathtracerpython_amd import _native, scene_reader
    from pathtracerpython_amd._abi import make_adapt
    from pathtracerpython_amd.adaptive import Accumulator
    from pathtracerpython_amd.render import Renderer
    from pathtracerpython_amd.synth import write_k5_scene
    scene_reader.VERBOSE = False
    k5 = scene_reader.Scene(write_k5_scene(tempfile.mkdtemp(), n_tris=100_000, seed=0, size=W))
    ms = {f: [] for f in FORMS}
    with Renderer(k5) as r:
        adapt = make_adapt(0.0, SPP, SPP, SPP)   # one pass: SPP samples to every pixel
        with Accumulator(r, W, H) as acc:
            for i in range(launches + 1):
                for aa in (False, True):
                    p = r.params(W, H, SPP, BOUNCES, SEED, aa=aa, kernel_times=True)
                    _, st = r.render_params(p, stats=True)
                    acc.reset()
                    acc.select(adapt)
                    sl = acc.render(p, adapt, stats=True)
                    if i:   # (the first round warms up)
                        ms["k_wf_shade_aa" if aa else "k_wf_shade"].append(st["shade_ms"])
                        ms["k_wf_shade_list_aa" if aa else "k_wf_shade_list"].append(sl["shade_ms"])
    print(json.dumps({"build_id": _native.build_id(), "shade_ms": {f: statistics.median(ms[f]) for f in FORMS}}))


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
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refactor_wf_shade.json"))
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args.launches)
    if not args.other_lib:
        raise SystemExit("--other-lib: the library to compare against")
    envs = {"other": dict(os.environ, PT_HIP_LIB=os.path.abspath(args.other_lib), PT_ALLOW_FOREIGN_BUILD="1"),
            "this": {k: v for k, v in os.environ.items() if k not in ("PT_HIP_LIB", "PT_ALLOW_FOREIGN_BUILD")}}
    bench = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "k5", "--no-cpu-baseline",
             "--no-check", "--no-secondary"]
    shade = [sys.executable, os.path.abspath(__file__), "--child", "--launches", str(args.launches)]
    rows = {t: {n: [] for n in ("k5_ms_per_step",) + FORMS} for t in envs}
    ids = {}
    for _ in range(args.rounds):
        for t, env in envs.items():
            b = run(bench, env, 600)
            s = run(shade, env, 300)
            ids[t] = s["build_id"]   # (bench.py loads the same library: _native.LIB_PATH)
            rows[t]["k5_ms_per_step"].append(b["ms_per_step"])
            for f in FORMS:
                rows[t][f].append(s["shade_ms"][f])
    res = {"shape": {"k5_ms_per_step": "bench.py --gpus 1 --config k5 (its default steps and warm-up)",
                     "shade_ms": {"scene": "K5 synth", "n_tris": 100_000, "width": W, "height": H, "spp": SPP,
                                  "bounces": BOUNCES, "seed": SEED, "launches": args.launches}},
           "rounds": args.rounds, "build_id": ids, "numbers": {}}
    for n in rows["this"]:
        o, t = stat(rows["other"][n]), stat(rows["this"][n])
        res["numbers"][n] = {"other": o, "this": t,
                             "this_median_inside_other_spread": bool(o["min"] <= t["median"] <= o["max"])}
    text = json.dumps(res, indent=1)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
