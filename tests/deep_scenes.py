"""Deep-stack scenes: Cornell variants with one extra mesh whose 4-wide BVH
walks hold many stack entries at once, or whose tree is too deep for the walk
kernels' stacks at all.

The wavefront walk kernels (pt_hip.hip k_wf_shadow / k_wf_closest) keep the
top kWalkStackLds = 16 entries of a lane's stack in shared memory and entries
16 .. 47 in a global overflow buffer with another stride (pt_path.h
ShadowStackT / ClosestStackT, the `top + 3 <= nl` switch of push3 /
push3_ref).  A scene whose `qstack` (pt_prepare.h: the entries a 4-wide walk
can need) exceeds kWalkStack = 48 is rendered by the single kernel instead.
Ordinary test scenes never hold 16 entries: a ray leaves most sibling boxes
untouched.  Two generators:

  sliver_scene  long thin triangles between two uniform points of the room:
                room-sized, heavily overlapping boxes.  A ray enters most
                sibling boxes and rarely hits a triangle, so the walks push
                three children at node after node and pop few of them early:
                peak occupancies of 20 and more (tests/test_deep_bvh_host.py
                pins them), every frame with thousands of node visits above
                the shared-memory part.
  comb_scene    a geometric comb: triangle i has size 2.5 r^i and sits at
                distance ~ r^i from one end of the room, so the SAH builder
                peels one triangle per level.  `qstack` grows with n and
                1 / (1 - r) until double precision ends the peeling.
                COMB_BELOW and COMB_ABOVE are the (n, r, axis) found nearest
                to the fallback bound from each side: qstack 48 (the walk
                kernels take it) and qstack 49 (the single kernel must).

Both write plain v/f OBJ text next to a copy of the Cornell files, as
conftest.random_scene does, and return the parsed scene."""
import os
import shutil

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CORNELL = os.path.join(ROOT, "scenes", "cornell", "cornellroom.sdl")
DEEP_MAT = "0.2 0.5 0.9 0.3 0.6 0.4 0 3"
WALK_STACK = 48        # kWalkStack (pt_hip.hip) = kBvhStack (pt_path.h)
WALK_STACK_LDS = 16    # kWalkStackLds: PT_WALK_STACK_LDS

# (n, r, axis): see comb_scene.  Found by a search over n = 100, 150 .. 400
# and r = 0.80 .. 0.97 along both axes (qstack from hc_bvh_info; 70 combs gave
# 26 .. 58): the same comb is on the bound along x and one past it along z.
COMB_BELOW = (200, 0.92, "x")   # qstack 48, bvh_depth 17
COMB_ABOVE = (200, 0.92, "z")   # qstack 49, bvh_depth 17
# The comb frames (W, H, spp, bounces, seed).  The z comb faces the camera on
# its axis, so three planes through the eye hold exact ties of the reference's
# own arithmetic, which the last bit of any evaluation order breaks its way
# (comb_frame_is_generic checks a frame for all three):
#   x + y = 0  holds every z-comb hypotenuse, and the primary rays of a square
#              image's anti-diagonal pixels: such a ray meets every triangle
#              exactly on an edge, where the sign of in_triangle's cross
#              products is rounding noise (20 x 20: three pixels 0.78 from the
#              oracle in the BVH and the no-BVH lane code alike).  With W - 1
#              and H - 1 coprime only the corner rays are in that plane, far
#              outside the triangles.
#   y = 0      the centre row of an odd H.  Its primary hits on the comb have
#              y = 0 exactly, the room's floor and ceiling are at y = -+3.8416
#              and intersect() meets lines, not half lines: the bounce ray's
#              line meets floor and ceiling at the same squared distance, and
#              the closer one is a matter of the last bit (20 x 17: the
#              device's Newton rsqrt and 1 / sqrt differ in the last bit of one
#              direction, the next hit moves from the floor to the ceiling,
#              one pixel 4.96e-05 from the oracle on the GPU).
#   x = 0      the centre column of an odd W, likewise between the side walls
#              at x = -+3.822.
COMB_FRAME = (20, 16, 2, 4, 9)


def comb_frame_is_generic(W, H):
    """No primary ray through an interior pixel lies in x + y = 0, x = 0 or
    y = 0, nor within 1e-9 of one (np.linspace pixel coordinates; the pixel
    spacing is 0.1 at these sizes)."""
    def lin(n, i):
        return -1.0 if n == 1 else (1.0 if i == n - 1 else i * (2.0 / (n - 1)) + -1.0)
    xs = [lin(W, i) for i in range(W)]
    ys = [lin(H, i) for i in range(H)]
    if min(abs(v) for v in xs + ys) < 1e-9:
        return False
    return not any(abs(x + y) < 1e-9 and abs(x) < 1.0 for x in xs for y in ys)


def _write(tmp_path, name, tris, fmt):
    """Cornell + the triangles (n, 3, 3) as object `name`, parsed."""
    src = os.path.dirname(CORNELL)
    for f in os.listdir(src):
        shutil.copy(os.path.join(src, f), tmp_path / f)
    line = "v " + " ".join([fmt] * 3)
    lines = [line % tuple(v) for t in tris for v in t]
    lines += ["f %d %d %d" % (3 * i + 1, 3 * i + 2, 3 * i + 3) for i in range(len(tris))]
    (tmp_path / name).write_text("\n".join(lines) + "\n")
    sdl = open(CORNELL).read().replace(
        "output cornell.pnm", "object %s %s\noutput cornell.pnm" % (name, DEEP_MAT))
    (tmp_path / "scene.sdl").write_text(sdl)
    from pathtracerpython_amd import scene_reader
    scene_reader.VERBOSE = False
    return scene_reader.Scene(str(tmp_path / "scene.sdl"))


def sliver_triangles(n=3000, seed=5, width=1e-2):
    """(n, 3, 3): triangle i is a, b, (a + b) / 2 + N(0, width), a and b
    uniform in the room."""
    rs = np.random.RandomState(seed)
    lo, hi = [-3.4, -3.4, -32.0], [3.4, 3.4, -17.5]
    out = np.empty((n, 3, 3))
    for i in range(n):
        a = rs.uniform(lo, hi)
        b = rs.uniform(lo, hi)
        out[i] = a, b, (a + b) / 2 + rs.normal(0, width, 3)
    return out


def sliver_scene(tmp_path, n=3000, seed=5, width=1e-2):
    return _write(tmp_path, "sliver.obj", sliver_triangles(n, seed, width), "%.9f")


def comb_triangles(n, r, axis):
    """(n, 3, 3): half squares of size s = 2.5 r^i, at z = -31.5 + 13.5 r^i
    (axis "z") or at x = -3.3 + 6.4 r^i around z = -25 (axis "x"), each
    tilted by 0.25 s out of its plane."""
    assert axis in ("x", "z")
    assert r ** n > 1e-9, "collapsed triangles (scene_reader.calc_normal divides by zero)"
    out = np.empty((n, 3, 3))
    for i in range(n):
        s = 2.5 * r ** i
        if axis == "z":
            z = -31.5 + 13.5 * r ** i
            out[i] = (-s, -s, z), (s, -s, z), (-s, s, z + 0.25 * s)
        else:
            x = -3.3 + 6.4 * r ** i
            out[i] = (x, -s, -25.0 - s), (x, s, -25.0 - s), (x + 0.25 * s, -s, -25.0 + s)
    return out


def comb_scene(tmp_path, n, r, axis):
    return _write(tmp_path, "comb.obj", comb_triangles(n, r, axis), "%.12f")
