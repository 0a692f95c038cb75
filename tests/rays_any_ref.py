"""Rays of any direction and origin (pt_radiance, include/pt_capi.h) — TEST
INFRASTRUCTURE shared by tests/test_rays_any_host.py and
tests/test_gpu_rays_any.py.

tests/rays_ref.py reaches the oracle through a descriptor with eye = o and a
one-point screen window, which only gives rays that cross z = 0 going forward
with d = p - o.  Here the reference is oracle.radiance (pt_oracle.c
oracle_radiance: path_body on (o, d, eye = o, key, sample)), and `restate` is
the same rule written again in Python from the oracle's primitives
(intersect_objects, compute_color, diffuse_dir, rotate) and
philox_ref.keyed_u, operation by operation in pt_oracle.c's order, so the C
entry is not taken at its word.  (diffuse_dir, main.py:242-247, is a primitive
because the compiler fuses sin and cos of one angle into a sincos call, whose
last bit is not always math.sin's and math.cos's.)

The ray classes, built per scene from fixed seeds (CLASS_NAMES, in the order
they are concatenated; `Rays.cat` is 257 records):
  inside    look_at_rays from (1, 0.5, -18) to (0, -1, -30), fov 60: unit
            directions from inside the room, o.z < 0 and d.z < 0, and five
            more towards points of the light.  No record of it escapes: the
            reference intersects lines, and a line from inside the room meets
            a wall one way or the other unless it runs through an edge
            exactly, where the last bit of in_triangle's cross products
            decides (tests/grazing.py: nothing sits on a boundary)
  outside   look_at_rays from (2.5, 1.5, 4) to (0, 0, -24), fov 40, and unit
            directions towards points of the light and of the specular objects
  ortho     ortho_rays towards a point of the light: one direction, an origin
            per record over a window wider than the room (the records' box
            is rays_box of them)
  axis      the six axis directions, twelve with one zero component, and
            directions with one component of 1e-30, 1e-39, 1e-42, 1e-45
            (subnormal or zero in f32) and 1e-200
  flat      d.z = 0, from inside the room and from in front of it
  length    one set of directions scaled by 1e30, 1e-30, 1e160 and 1e-160
  surface   origins at centroids, edge midpoints and vertices of triangles of
            walls, cubes and meshes (the sqd > 1e-5 rule for a primary ray)
  far       origins 30 to 200 from the room, aimed into it
and, apart from them, `overflow`: lengths of 1e300 and 1e-300, where the
reference's own norm overflows or underflows and every record's value is 0.
"""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from philox_ref import keyed_u  # noqa: E402

BOUNCES, SEED = 3, 9
INSIDE = dict(eye=(1.0, 0.5, -18.0), target=(0.0, -1.0, -30.0), fov_y=60.0)
OUTSIDE = dict(eye=(2.5, 1.5, 4.0), target=(0.0, 0.0, -24.0), fov_y=40.0)
ORTHO = dict(eye=(0.5, -3.0, 4.0), width=11.0)
GRID = (7, 5)
CLASS_NAMES = ("inside", "outside", "ortho", "axis", "flat", "length", "surface", "far")
CAMERAS = CLASS_NAMES[:3]
N_CAT = 257
TINY = (1e-30, 1e-39, 1e-42, 1e-45, 1e-200)
SCALES = (1e30, 1e-30, 1e160, 1e-160)
# samples 0 .. SPEC_SAMPLES-1 decide whether a record counts as one whose bounce 0
# takes the specular branch (every test renders at least these)
SPEC_SAMPLES = 5
TOL, TOL32 = 1e-12, 1e-6
# the host lane code's largest difference from oracle.radiance per class over
# the three host scenes (mean, S and Q at 5 spp, relative to max(1, |value|)),
# measured on the CPU by tests/test_rays_any_host.py; the tolerance of a class
# is frames.oracle_tol's rule: 8 x that, with the project's 1e-12 as the floor
MEASURED = {"inside": 1.44e-15, "outside": 1.06e-15, "ortho": 2.11e-15, "axis": 8.59e-16, "flat": 7.77e-16,
            "length": 2.91e-15, "surface": 1.83e-15, "far": 1.60e-14, "overflow": 0.0}


def class_tol(name):
    return max(8.0 * MEASURED[name], TOL)


def rel(got, want):
    """Largest difference relative to max(1, |value|)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if got.size == 0:
        return 0.0
    return float((np.abs(got - want) / np.maximum(1.0, np.abs(want))).max())


# ------------------------------------------------------- the restatement --
def _f(x):
    return np.float64(x)


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _unit(a):
    n = _f(math.sqrt(_dot(a, a)))
    return [a[0] / n, a[1] / n, a[2] / n]


def _pow(x, y):
    try:
        return _f(math.pow(x, y))
    except (ValueError, OverflowError):
        return _f(np.power(_f(x), _f(y)))


def restate(pk, origins, dirs, keys, bounces, seed, n_samples, sample_begin=0, rr_depth=None):
    """(colours [n_samples, n, 3], spec0 [n_samples, n] bool): main.py:186-271
    per record and sample from the oracle's primitives, with the eye of the
    specular term at the record's origin; spec0 marks the samples whose bounce
    0 takes the specular branch.  Every f64 operation is one numpy scalar
    operation, in pt_oracle.c path_body's order."""
    from oracle import oracle
    o_all = np.asarray(origins, dtype=np.float64).reshape(-1, 3)
    d_all = np.asarray(dirs, dtype=np.float64).reshape(-1, 3)
    mat = np.asarray(pk.mat, dtype=np.float64).reshape(-1, 8)
    tri_n = np.asarray(pk.tri_n, dtype=np.float64).reshape(-1, 3)
    tri_obj = np.asarray(pk.tri_obj)
    light = [_f(v) for v in pk.light_rgb]
    n = o_all.shape[0]
    out = np.zeros((n_samples, n, 3))
    spec0 = np.zeros((n_samples, n), dtype=bool)
    zero, one = _f(0.0), _f(1.0)
    with np.errstate(all="ignore"):
        for i in range(n):
            key = int(keys[i])
            for j in range(n_samples):
                s = sample_begin + j
                o = [_f(v) for v in o_all[i]]
                eye = list(o)
                d = [_f(v) for v in d_all[i]]
                k = one
                rgb = [zero, zero, zero]
                for b in range(bounces):
                    t, P = oracle.intersect_objects(pk, np.array([o + d], dtype=np.float64))
                    t, P = int(t[0]), [_f(v) for v in P[0]]
                    if t < 0:
                        break
                    if t >= pk.n_obj_tri:
                        rgb = [rgb[c] + light[c] * k for c in range(3)]
                        break
                    obj = int(tri_obj[t])
                    nrm = [_f(v) for v in tri_n[t]]
                    m = [_f(v) for v in mat[obj]]
                    u = [_f(keyed_u(seed, key, s, b, q)) for q in range(16)]
                    col = oracle.compute_color(pk, [obj], np.array([P]), np.array([nrm]), np.array([u[:12]]))[0]
                    rgb = [rgb[c] + _f(col[c]) * k for c in range(3)]
                    xi = zero + ((m[4] + m[5]) - zero) * u[12]
                    if xi <= m[4]:
                        nd = [_f(x) for x in oracle.rotate(np.array(nrm), oracle.diffuse_dir(u[13], u[14]))]
                        k = k * (m[4] * _dot(nd, nrm))
                    else:
                        if b == 0:
                            spec0[j, i] = True
                        ndd = _dot(nrm, d)
                        r = _unit([ndd * 2 * nrm[c] - d[c] for c in range(3)])
                        e = _unit([eye[c] - P[c] for c in range(3)])
                        nd = [_f(x) for x in oracle.rotate(np.array(nrm), np.array(r))]
                        k = k * (m[5] * _pow(_dot(e, nd), m[7]))
                    if rr_depth is not None and b >= rr_depth:
                        q = abs(k)
                        q = _f(0.05) if q < 0.05 else (one if q > 1.0 else q)
                        if u[15] >= q:
                            break
                        k = k / q
                    o, d = P, nd
                out[j, i] = rgb
    return out, spec0


# ------------------------------------------------------------ the classes --
def room(pk):
    """(lo, hi) of the object triangles' vertices."""
    v = np.asarray(pk.tri_v, dtype=np.float64).reshape(-1, 3)[:3 * pk.n_obj_tri]
    return v.min(axis=0), v.max(axis=0)


def light_points(pk, rng, n):
    lv = np.asarray(pk.tri_v, dtype=np.float64).reshape(-1, 3, 3)[pk.n_obj_tri:]
    return np.array([rng.dirichlet([1.0, 1.0, 1.0]) @ lv[rng.integers(len(lv))] for _ in range(n)])


def towards(o, points):
    """Unit directions from o to the points, as look_at_rays forms its own."""
    d = np.asarray(points, dtype=np.float64) - np.asarray(o, dtype=np.float64)
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def specular_points(pk, rng, n):
    """n points of triangles whose material has ks > 0."""
    v = np.asarray(pk.tri_v, dtype=np.float64).reshape(-1, 3, 3)
    ks = np.asarray(pk.mat, dtype=np.float64).reshape(-1, 8)[:, 5]
    tris = np.flatnonzero(ks[np.asarray(pk.tri_obj)[:pk.n_obj_tri]] > 0)
    return np.array([rng.dirichlet([1.0, 1.0, 1.0]) @ v[rng.choice(tris)] for _ in range(n)])


def first_tri(pk, o, d):
    from oracle import oracle
    o = np.broadcast_to(np.asarray(o, dtype=np.float64), np.shape(d))
    return np.asarray(oracle.intersect_objects(pk, np.concatenate([o, d], axis=1))[0])


def light_aimed(pk, eye, rng, n, tries=3000):
    """n unit directions from `eye` towards points of the light whose first
    hit, by the reference, is the light (other triangles may stand between)."""
    d = towards(eye, light_points(pk, rng, tries))
    d = d[first_tri(pk, eye, d) >= pk.n_obj_tri]
    assert len(d) >= n, "the light cannot be seen from the eye"
    return d[:n]


def camera_class(pk, which, rng):
    from pathtracerpython_amd import cameras
    W, H = GRID
    if which == "ortho":   # towards the first point of the light that gives some record a light hit
        for target in light_points(pk, rng, 200):
            o, d, _ = cameras.ortho_rays(ORTHO["eye"], target, width=ORTHO["width"], W=7, H=7)
            if (first_tri(pk, o, d) >= pk.n_obj_tri).any():
                return o, d
        raise AssertionError("no ortho view reaches the light")
    cam = INSIDE if which == "inside" else OUTSIDE
    o, d, _ = cameras.look_at_rays(cam["eye"], cam["target"], fov_y=cam["fov_y"], W=W, H=H)
    extra = [light_aimed(pk, cam["eye"], rng, 5 if which == "inside" else 3)]
    if which == "outside":
        extra.append(towards(cam["eye"], specular_points(pk, rng, 5)))
    d = np.concatenate([d] + extra)
    return np.broadcast_to(np.asarray(cam["eye"], dtype=np.float64), d.shape).copy(), d


def axis_class(pk, rng):
    d = []
    for a in range(3):
        for s in (1.0, -1.0):
            v = np.zeros(3)
            v[a] = s
            d.append(v)
    for a in range(3):   # one zero component, the others of either sign
        for s, t in ((1.0, 1.0), (1.0, -1.0), (-1.0, 1.0), (-0.5, -2.0)):
            v = np.array([s, t])
            d.append(np.insert(v, a, 0.0))
    for i, tiny in enumerate(TINY):   # one tiny component
        for a in range(3):
            v = np.array([0.6, -0.8]) * (1.0 if (i + a) % 2 else -1.0)
            d.append(np.insert(v, a, tiny if a != 1 else -tiny))
    d = np.array(d)
    inside = np.array([INSIDE["eye"], (-1.5, 1.25, -24.0)])
    o = inside[np.arange(len(d)) % 2]
    return o, d


def flat_class(pk, rng, n=16):
    a = (np.arange(n) + 0.37) * (2 * np.pi / n)
    d = np.stack([np.cos(a), np.sin(a), np.zeros(n)], axis=1)
    lo, hi = room(pk)
    o = rng.uniform(lo + 0.3, hi - 0.3, size=(n, 3))
    o[::4] = rng.uniform([-6, -6, 1.0], [6, 6, 3.0], size=(len(o[::4]), 3))   # in front of the room: escapes
    return o, d


def length_class(pk, rng, n=6):
    """n directions, half of them towards points of the specular objects, from
    the inside and the outside eye in turn, at each of SCALES."""
    lo, hi = room(pk)
    o = np.array([INSIDE["eye"], OUTSIDE["eye"]])[np.arange(n) % 2]
    base = np.concatenate([rng.uniform(lo, hi, size=(n - n // 2, 3)), specular_points(pk, rng, n // 2)]) - o
    return np.concatenate([o] * len(SCALES)), np.concatenate([base * s for s in SCALES])


def takes_specular(pk, tri, key, sample=0):
    """Whether bounce 0 of `sample` of a record with first hit `tri` and pixel
    word `key` takes the specular branch: uniform(0, kd + ks) > kd, slot 12."""
    if tri < 0 or tri >= pk.n_obj_tri:
        return False
    m = np.asarray(pk.mat, dtype=np.float64).reshape(-1, 8)[int(np.asarray(pk.tri_obj)[tri])]
    return bool(0.0 + ((m[4] + m[5]) - 0.0) * keyed_u(SEED, int(key), sample, 0, 12) > m[4])


def length_keys(pk, o, d, rng):
    """One key per direction, the same at every scale, so that a direction's
    draws are the same whatever its length; where the first hit's material has
    a specular part the key is stepped until sample 0 takes that branch — the
    only place where the length of d shows."""
    n = len(o) // len(SCALES)
    keys = rng.integers(0, 1 << 31, size=n, dtype=np.uint64)
    tri = first_tri(pk, o[:n], d[:n])
    ks = np.asarray(pk.mat, dtype=np.float64).reshape(-1, 8)[:, 5]
    for j in range(n):
        if 0 <= tri[j] < pk.n_obj_tri and ks[np.asarray(pk.tri_obj)[tri[j]]] > 0:
            while not takes_specular(pk, tri[j], keys[j]):
                keys[j] += 1
    return np.tile(keys, len(SCALES)).astype(np.uint32)


def surface_triangles(pk, rng, n=6):
    """n object triangles: one of the first object without a specular part,
    one of each object with one (cubes, meshes; at most 4), the rest drawn."""
    tri_obj = np.asarray(pk.tri_obj)[:pk.n_obj_tri]
    ks = np.asarray(pk.mat, dtype=np.float64).reshape(-1, 8)[:, 5]
    objs = [int(np.flatnonzero(ks == 0)[0])] + [int(x) for x in np.flatnonzero(ks > 0)[:4]]
    tris = [int(rng.choice(np.flatnonzero(tri_obj == x))) for x in objs]
    while len(tris) < n:
        t = int(rng.integers(pk.n_obj_tri))
        if t not in tris:
            tris.append(t)
    return tris[:n]


def hit_gap(pk, o, d):
    """(sqd2 - sqd1) / sqd1 of the two nearest hits on the line (o, d) that
    the reference's closest-hit search weighs (sqd > 1e-5, utils.py:98-147 per
    triangle through oracle.intersect); inf with fewer than two.  Triangles
    that are exact copies of an earlier one are left out (the mesh golden holds
    duplicates: their tie goes to the first, by index)."""
    from oracle import oracle
    v = np.asarray(pk.tri_v, dtype=np.float64).reshape(-1, 3, 3)
    seen, sq = set(), []
    for t in v:
        key = t.tobytes()
        if key in seen:
            continue
        seen.add(key)
        h, Q = oracle.intersect(t, o, d)
        if h:
            x = float(np.sum((Q - o) ** 2))
            if x > 1e-5:
                sq.append(x)
    sq.sort()
    return np.inf if len(sq) < 2 else (sq[1] - sq[0]) / sq[0]


MIN_GAP = 1e-9   # no record's closest hit is a tie for the last bits to decide


def surface_class(pk, rng):
    """Two directions from the centroid, an edge's midpoint and a vertex of
    each of surface_triangles.  A point and a direction are drawn again while
    the two nearest hits are within 1e-6 of each other: the midpoint of a
    cube's upright edge is as far from the floor as from the cube's top,
    whatever the direction."""
    v = np.asarray(pk.tri_v, dtype=np.float64).reshape(-1, 3, 3)
    o, d = [], []
    for t in surface_triangles(pk, rng):
        a, b, c = v[t]
        for kind in range(3):
            for _ in range(2):
                for _ in range(50):
                    e = int(rng.integers(3))
                    p = ((a + b + c) / 3.0, 0.5 * (v[t][e] + v[t][(e + 1) % 3]), v[t][e])[kind]
                    q = rng.normal(size=3)
                    if hit_gap(pk, p, q) > 1e-6:
                        break
                else:
                    raise AssertionError("no well-posed ray from triangle %d" % t)
                o.append(p)
                d.append(q)
    return np.array(o), np.array(d)


def far_class(pk, rng, n):
    lo, hi = room(pk)
    c = 0.5 * (lo + hi)
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    R = np.array([30.0, 100.0, 200.0])[np.arange(n) % 3]
    o = c + u * R[:, None]
    return o, rng.uniform(lo + 0.2, hi - 0.2, size=(n, 3)) - o


def overflow_class(pk, rng, n=4):
    lo, hi = room(pk)
    o = np.array([INSIDE["eye"], OUTSIDE["eye"]])[np.arange(n) % 2]
    base = rng.uniform(lo, hi, size=(n, 3)) - o
    return np.concatenate([o, o]), np.concatenate([base * 1e300, base * 1e-300])


class Rays:
    """A scene's classes: name -> (o, d, keys), their concatenation `cat`
    (N_CAT records, `spans` the slice of each class), the box of the ortho
    class's origins and the inside eye (`box`: the other origins stay outside
    it), and the reference's samples, computed once and shared."""

    def __init__(self, scene, seed=11):
        from pathtracerpython_amd import cameras
        from pathtracerpython_amd.pack import pack_scene
        self.scene = scene
        self.pk = pack_scene(scene)
        rng = np.random.default_rng(seed)
        parts = {}
        for name in CAMERAS:
            parts[name] = camera_class(self.pk, name, rng)
        parts["axis"] = axis_class(self.pk, rng)
        parts["flat"] = flat_class(self.pk, rng)
        parts["length"] = length_class(self.pk, rng)
        parts["surface"] = surface_class(self.pk, rng)
        parts["far"] = far_class(self.pk, rng, N_CAT - sum(len(v[0]) for v in parts.values()))
        self.classes, self.spans = {}, {}
        at = 0
        for name in CLASS_NAMES:
            o, d = (np.ascontiguousarray(x, dtype=np.float64) for x in parts[name])
            keys = rng.integers(0, 1 << 32, size=len(o), dtype=np.uint64).astype(np.uint32)
            if name == "length":
                keys = length_keys(self.pk, o, d, rng)
            self.classes[name] = (o, d, keys)
            self.spans[name] = slice(at, at + len(o))
            at += len(o)
        assert at == N_CAT
        self.o, self.d, self.keys = (np.concatenate([self.classes[c][i] for c in CLASS_NAMES]) for i in range(3))
        o, d = overflow_class(self.pk, rng)
        self.overflow = (o, d, rng.integers(0, 1 << 32, size=len(o), dtype=np.uint64).astype(np.uint32))
        lo, hi = cameras.rays_box(np.concatenate([self.classes["ortho"][0], [INSIDE["eye"]]]))
        self.box = np.concatenate([lo, hi])
        self._ref = {}

    def records(self, name):
        return self.overflow if name == "overflow" else self.classes[name]

    def samples(self, name="cat", rr_depth=None, s0=0, ns=8):
        """oracle.radiance's [ns, n, 3] of class `name` ("cat": all 257)."""
        from oracle import oracle
        from pathtracerpython_amd._abi import PT_FLAG_RR
        key = (name, rr_depth, s0, ns)
        if key not in self._ref:
            o, d, k = (self.o, self.d, self.keys) if name == "cat" else self.records(name)
            self._ref[key] = oracle.radiance(self.pk, o, d, k, BOUNCES, SEED, ns, s0,
                                             0 if rr_depth is None else PT_FLAG_RR,
                                             3 if rr_depth is None else rr_depth)
        return self._ref[key]

    def restated(self):
        """restate's (colours, spec0) of all 257 records, SPEC_SAMPLES samples."""
        if "restated" not in self._ref:
            self._ref["restated"] = restate(self.pk, self.o, self.d, self.keys, BOUNCES, SEED, SPEC_SAMPLES)
        return self._ref["restated"]

    def coverage(self):
        """name -> (escapes, light hits, records whose bounce 0 takes the
        specular branch in one of the first SPEC_SAMPLES samples), from the
        reference: the first hits by oracle.intersect_objects, the branch by
        the rule's own draw uniform(0, kd + ks) > kd (slot 12 of bounce 0)."""
        from oracle import oracle
        tri = np.asarray(oracle.intersect_objects(self.pk, np.concatenate([self.o, self.d], axis=1))[0])
        mat = np.asarray(self.pk.mat, dtype=np.float64).reshape(-1, 8)
        solid = (tri >= 0) & (tri < self.pk.n_obj_tri)
        obj = np.asarray(self.pk.tri_obj)[np.where(solid, tri, 0)]
        spec = np.zeros(len(tri), dtype=bool)
        for i in np.flatnonzero(solid & (mat[obj, 5] > 0)):
            kd, ks = mat[obj[i], 4], mat[obj[i], 5]
            spec[i] = any(0.0 + ((kd + ks) - 0.0) * keyed_u(SEED, int(self.keys[i]), s, 0, 12) > kd
                          for s in range(SPEC_SAMPLES))
        return {c: (int((tri[sl] < 0).sum()), int((tri[sl] >= self.pk.n_obj_tri).sum()), int(spec[sl].sum()))
                for c, sl in self.spans.items()}

    def check_coverage(self):
        """The condition the comparisons rest on, asserted from the reference:
        every camera class holds a light hit and three records whose bounce 0
        takes the specular branch — the only place where the sign and the
        length of d and the eye = o of the rule show — and the two cameras
        outside the room an escape (see `inside` above)."""
        gap = min(hit_gap(self.pk, self.o[i], self.d[i]) for i in range(N_CAT))
        print(f"smallest relative gap between a record's two nearest hits: {gap:.2e}")
        assert gap >= MIN_GAP
        cov = self.coverage()
        print("coverage (escapes, light hits, specular bounce 0): " +
              ", ".join(f"{c} {cov[c]}" for c in CLASS_NAMES))
        assert cov["length"][2] >= 3   # (a specular bounce 0 at 1e30, 1e-30 and 1e-160; 1e160 escapes: its norm is inf)
        for c in CAMERAS:
            esc, lit, spec = cov[c]
            assert (esc >= 1 or c == "inside") and lit >= 1 and spec >= 3, (c, cov[c])
        # the branch as `restate` took it is the branch as coverage() draws it
        spec0 = self.restated()[1].any(axis=0)
        for c in CAMERAS:
            assert int(spec0[self.spans[c]].sum()) == cov[c][2]
        return cov


_made = {}


def rays_of(name, make):
    """The process-wide Rays of scene `name`; make() builds the scene."""
    if name not in _made:
        _made[name] = Rays(make())
    return _made[name]


# ------------------------------------------------------------ the goldens --
# (fixture, scene, camera, records): tests/golden/gen_golden.py `rays` runs the
# unmodified reference on these; one origin per fixture (the reference's eye)
GOLDEN_GRID = (5, 4)
GOLDENS = (("rays_cornell_inside.npz", "cornell", "inside"), ("rays_cornell_outside.npz", "cornell", "outside"),
           ("rays_mesh_inside.npz", "mesh", "inside"))
GOLDEN_FRAME = (2, 3, 9)   # spp, bounces, seed


def golden_rays(camera):
    """(o [3], d [n, 3]): a look_at_rays grid, the six axis directions, one
    direction with d.z = 0 and two of the grid's scaled by 1e10 and 1e-9."""
    from pathtracerpython_amd import cameras
    cam = INSIDE if camera == "inside" else OUTSIDE
    W, H = GOLDEN_GRID
    _, d, _ = cameras.look_at_rays(cam["eye"], cam["target"], fov_y=cam["fov_y"], W=W, H=H)
    axes = np.concatenate([np.eye(3), -np.eye(3)])
    flat = np.array([[0.8, -0.6, 0.0]])
    scaled = np.array([d[6] * 1e10, d[13] * 1e-9])
    return np.asarray(cam["eye"], dtype=np.float64), np.concatenate([d, axes, flat, scaled])
