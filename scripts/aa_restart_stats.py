#!/usr/bin/env python3
"""How often a wave of k_render_aa runs the restart's closest query (dev tool,
CPU only): the kernel's lane code on the host (tests/hostcheck/pt_aa_host.cpp,
hc_aa_restart_stats), the lanes of a frame grouped into waves of 64 in launch
order.

    python3 scripts/aa_restart_stats.py [--size 128] [--spp 64] [--bounces 4] [--lanes 16]

Prints one JSON line: per wave, the loop iterations, the restart queries it
runs (an iteration costs the most queries any of its lanes needs), the lockstep
floor (the samples of a lane), and the lane utilisation of the loop."""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hostlib  # noqa: E402  (tests/hostlib.py: the hostcheck Makefile's rule)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--bounces", type=int, default=4)
    ap.add_argument("--lanes", type=int, default=16)
    ap.add_argument("--seed", type=int, default=9)
    a = ap.parse_args()
    from pathtracerpython_amd import scene_reader
    from pathtracerpython_amd._abi import PT_FLAG_AA, make_params
    from pathtracerpython_amd.pack import pack_scene
    scene_reader.VERBOSE = False
    lib = hostlib.build(tempfile.mkdtemp(), "pt_aa_host")
    pk = pack_scene(scene_reader.Scene(os.path.join(ROOT, "scenes", "cornell", "cornellroom.sdl")))
    p = make_params(a.size, a.size, a.spp, a.bounces, a.seed, PT_FLAG_AA)
    v = (C.c_int64 * 6)()
    rc = lib.hc_aa_restart_stats(C.byref(pk.desc), C.byref(p), a.lanes, v)
    if rc:
        raise SystemExit(f"hc_aa_restart_stats: {rc}")
    waves, iters, queries, it_restart, floor, lane_iters = (int(x) for x in v)
    print(json.dumps({
        "frame": [a.size, a.size], "spp": a.spp, "bounces": a.bounces, "lanes_per_pixel": a.lanes,
        "waves": waves, "iterations_per_wave": iters / waves, "restart_queries_per_wave": queries / waves,
        "lockstep_floor_queries_per_wave": floor / waves,
        "queries_over_floor": queries / floor,
        "share_of_iterations_with_a_restart": it_restart / iters,
        "loop_lane_utilisation": lane_iters / (64 * iters)}))


if __name__ == "__main__":
    main()
