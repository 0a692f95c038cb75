"""Reference frames of the thin lens on the mesh scene — TEST INFRASTRUCTURE
shared by tests/test_lens_wavefront_host.py and tests/test_gpu_lens_wavefront.py:
the oracle's per-sample colours through the lens (tests/lens_ref.py
lens_samples), computed once per session and shape, with the restart loop's
branch coverage (lens_ref.coverage: mixed-escape, mixed-light, all-escape)
asserted before anything is compared against them."""
import functools

import numpy as np

import lens_ref

from pathtracerpython_amd.pack import pack_scene

A, B = lens_ref.CASE_A, lens_ref.CASE_B
CASES = {"A": A, "B": B}
BOUNCES, SEED = 3, 5

_scene = {}


def use_scene(scene):
    """The mesh scene of the `mesh_golden` fixture (session-wide; the caches
    below are keyed by case and shape alone)."""
    _scene.setdefault("mesh", scene)
    return scene


@functools.lru_cache(maxsize=None)
def _samples(case, W, H, bounces, n, flags, rr_depth):
    c = lens_ref.lens_samples(_scene["mesh"], W, H, bounces, SEED, n, flags=flags, rr_depth=rr_depth, **CASES[case])
    c.setflags(write=False)
    return c


def samples(case, W=12, H=12, bounces=BOUNCES, n=8, flags=0, rr_depth=3):
    """Per-sample colours [n, W*H, 3] in list order (read-only, cached)."""
    return _samples(case, W, H, bounces, n, flags, rr_depth)


def covered(c, want, what):
    """Assert the branches `want` (a triple of bools) on list-order frames c."""
    cov = lens_ref.coverage(c, pack_scene(_scene["mesh"]).light_rgb)
    print(f"coverage {what}: mixed-escape {cov[0]}, mixed-light {cov[1]}, all-escape {cov[2]}")
    for got, need in zip(cov, want):
        assert got >= 1 or not need, f"{what}: coverage {cov}, wanted {want}"
    return cov


@functools.lru_cache(maxsize=None)
def frames(case):
    """The 12x12, 3 bounce, seed 5 fixture in image orientation [n, H, W, 3]:
    17 samples of A, 8 of B.  A: all three branches in the first 8, the first 2
    and all 17 samples; B (no jitter: no pixel mixes light and other samples):
    mixed-escape and all-escape in the first 8 and the first 2."""
    c = samples(case, n=17 if case == "A" else 8)
    light = case == "A"
    for n in ((8, 2, 17) if case == "A" else (8, 2)):
        covered(c[:n], (True, light, True), f"{case}, first {n} samples")
    out = lens_ref.to_image(c, 12, 12)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def frames_small(which):
    """A at 7x5, 8 samples (mixed-escape) and at 6x6, 64 samples, 2 bounces
    (mixed-escape and mixed-light)."""
    if which == "7x5":
        c = samples("A", 7, 5, n=8)
        covered(c, (True, False, False), "A 7x5, 8 samples")
        out = lens_ref.to_image(c, 7, 5)
    else:
        c = samples("A", 6, 6, bounces=2, n=64)
        covered(c, (True, True, False), "A 6x6, 64 samples, 2 bounces")
        out = lens_ref.to_image(c, 6, 6)
    out.setflags(write=False)
    return out


def sums(fr):
    """(sum, sum of squares) over the samples of frames [n, H, W, 3]."""
    fr = np.asarray(fr)
    return fr.sum(axis=0), (fr ** 2).sum(axis=0)
