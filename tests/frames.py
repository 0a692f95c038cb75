"""Scenes off the Cornell frame.  Every test scene otherwise lives where the
Cornell room does (coordinates up to ~19 about a centre near the origin); the
f32 filter's bounds and the BVH boxes' inflation all scale with that extent.
`transformed` gives the same scene scaled and shifted, `FRAMES` the list the
host and GPU tests share, `oracle_tol` the oracle tolerance of each."""
import numpy as np

from pathtracerpython_amd.pack import PackedScene


def transformed(packed, s, tx=0.0, ty=0.0):
    """`packed` scaled by s about the origin, then shifted by (tx, ty, 0):
    vertices, eye and the ortho window; areas scale with s^2, normals stay.
    There is no z shift: the screen plane is z = 0 in the oracle
    (pt_oracle.c: the screen point's z is 0.0) as in the kernels, and s * 0
    leaves it there.  Returns a new PackedScene with its own arrays and
    descriptor."""
    s, tx, ty = float(s), float(tx), float(ty)
    t = np.array([tx, ty, 0.0])
    q = object.__new__(PackedScene)
    q.n_obj_tri = packed.n_obj_tri
    q.n_obj = packed.n_obj
    q.tri_v = np.ascontiguousarray(packed.tri_v * s + t)
    q.tri_n = packed.tri_n.copy()
    q.tri_area = np.ascontiguousarray(packed.tri_area * (s * s))
    q.tri_obj = packed.tri_obj.copy()
    q.mat = packed.mat.copy()
    q.eye = packed.eye * s + t
    q.ortho = packed.ortho * s + np.array([tx, ty, tx, ty])
    q.ambient = packed.ambient
    q.light_rgb = packed.light_rgb.copy()
    q.desc = q._make_desc()
    return q


# (name, scale, x shift, y shift)
FRAMES = [
    ("x1e-3", 1e-3, 0.0, 0.0),
    ("x1e-2", 1e-2, 0.0, 0.0),
    ("x1e2", 1e2, 0.0, 0.0),
    ("x1e4", 1e4, 0.0, 0.0),
    ("x1e6", 1e6, 0.0, 0.0),
    ("shift1e3", 1.0, 1e3, -1e3),
    ("shift1e6", 1.0, 1e6, 1e6),
    ("x1e-2_shift1e4", 1e-2, 1e4, 0.0),
]
# the four the GPU tests render
GPU_FRAMES = ["x1e-2", "x1e4", "shift1e3", "x1e-2_shift1e4"]
FRAME = (12, 12, 2, 4, 8)   # W, H, spp, bounces, seed


def frame(name):
    return next(f for f in FRAMES if f[0] == name)


# Oracle tolerance of FRAME on each scene, relative to the frame's maximum.
# MEASURED is the host build's own difference from the oracle (IEEE against
# IEEE, both off the device: the conditioning of the scene's coordinates, which
# a shift by 1e6 makes ~1e-11), measured on the CPU with the hybrid render of
# tests/test_hostcheck.py, "mesh" = random_scene(300, 21).  The tolerance is
# 8 x that with a floor of 1e-12 (the suite's bar in the Cornell frame): the
# factor covers the device's faithfully rounded reciprocals (rcp_d, rsqrt_d,
# up to ~2 ulp) where the host has correctly rounded divisions (0.5 ulp).
MEASURED = {
    ("cornell", "x1e-3"): 7.611e-16, ("mesh", "x1e-3"): 1.201e-15,
    ("cornell", "x1e-2"): 9.701e-16, ("mesh", "x1e-2"): 7.468e-16,
    ("cornell", "x1e2"): 6.467e-16, ("mesh", "x1e2"): 4.528e-16,
    ("cornell", "x1e4"): 5.659e-16, ("mesh", "x1e4"): 6.791e-16,
    ("cornell", "x1e6"): 8.084e-16, ("mesh", "x1e6"): 1.075e-15,
    ("cornell", "shift1e3"): 1.692e-14, ("mesh", "shift1e3"): 2.111e-14,
    ("cornell", "shift1e6"): 2.790e-11, ("mesh", "shift1e6"): 1.517e-11,
    ("cornell", "x1e-2_shift1e4"): 6.517e-12, ("mesh", "x1e-2_shift1e4"): 5.664e-12,
}


def oracle_tol(scene, name):
    return max(8.0 * MEASURED[(scene, name)], 1e-12)


def rel_err(fb_list, ref):
    """L-inf difference divided by the reference frame's maximum."""
    return float(np.abs(fb_list - ref).max() / np.abs(ref).max())
