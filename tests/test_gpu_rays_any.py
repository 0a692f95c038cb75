"""Rays of any direction and origin on the GPU: the classes of
tests/rays_any_ref.py (unit directions of the shipped cameras, a camera inside
the room, zero and f32-subnormal components, d.z = 0, lengths of 1e+-30 and
1e+-160, origins on surfaces and far from the room) through
Renderer.render_rays — k_render_rays on a scene without a BVH, the wavefront
kernels and the single kernel on scenes with one — and through a ray
accumulator, against oracle.radiance (pt_oracle.c oracle_radiance, pinned on
the CPU by tests/test_rays_any_host.py) and against goldens of the unmodified
reference (tests/golden/rays_*.npz)."""
import os

import numpy as np
import pytest

import adaptive_sim
import conftest
import devcheck_lib
import rays_adaptive_ref as adaptive_ref
import rays_any_ref as ra
from conftest import GOLDEN
from oracle import oracle
from pathtracerpython_amd import cameras
from pathtracerpython_amd._abi import PT_PATH_SINGLE, PT_PATH_WAVEFRONT, make_adapt, make_params
from pathtracerpython_amd.adaptive import RayAccumulator
from pathtracerpython_amd.render import Renderer

pytestmark = pytest.mark.gpu

# (records, spp, rr_depth or None, sample_begin): prefixes of the 257 records
CASES = ((1, 5, None, 0), (63, 5, None, 0), (64, 8, None, 0), (65, 8, None, 0), (257, 5, None, 0),
         (65, 8, 1, 0), (63, 8, None, 5))
BVH_SCENES = ("mesh", "multi")


def cid(c):
    return "n%d-spp%d%s%s" % (c[0], c[1], "" if c[2] is None else "-rr%d" % c[2], "-s%d" % c[3] if c[3] else "")


def gpu():
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else a.dtype)


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


@pytest.fixture(scope="module")
def envs(tmp_path_factory, cornell, mesh_golden):
    """name -> (rays_any_ref.Rays, Renderer with its box, Renderer without);
    the coverage is asserted from the reference when a scene's rays are made."""
    gpu()
    made = {}

    def get(name):
        if name not in made:
            make = {"cornell": lambda: cornell, "mesh": lambda: mesh_golden[0],
                    "multi": lambda: conftest.multi_mesh_scene(tmp_path_factory.mktemp("multi"), 5)}[name]
            R = ra.rays_of(name, make)
            R.check_coverage()
            made[name] = (R, Renderer(R.scene, ray_box=(R.box[:3], R.box[3:])), Renderer(R.scene))
        return made[name]
    yield get
    for _, r, q in made.values():
        r.close()
        q.close()


def kw_of(spp, rr_depth, s0):
    return dict(spp=spp, bounces=ra.BOUNCES, seed=ra.SEED, rr=rr_depth is not None,
                rr_depth=3 if rr_depth is None else rr_depth, sample_begin=s0)


def moments(want):
    return want.sum(axis=0) / len(want), want.sum(axis=0), (want ** 2).sum(axis=0)


def per_class(R, n, got, want):
    """name -> largest difference (relative to max(1, |value|)) among the
    class's records within the first n."""
    out = {}
    for c, sl in R.spans.items():
        a, b = sl.start, min(sl.stop, n)
        if a < b:
            out[c] = max(ra.rel(g[a:b], w[a:b]) for g, w in zip(got, want))
    return out


def check_against_oracle(R, r, n, spp, rr_depth, s0, path, tag, **more):
    """render_rays of the first n records, with and without moments, 1 and 4
    lanes: every record within its class's tolerance of the oracle entry."""
    want = moments(R.samples("cat", rr_depth, s0, spp)[:, :n])
    kw = dict(kw_of(spp, rr_depth, s0), **more)
    for lanes in (1, 4):
        rgb = r.render_rays(R.o[:n], R.d[:n], R.keys[:n], lanes_per_pixel=lanes, **kw)
        assert r.last_launch()["path"] == path
        g, S, Q = r.render_rays(R.o[:n], R.d[:n], R.keys[:n], lanes_per_pixel=lanes, moments=True, **kw)
        assert r.last_launch()["path"] == path
        assert same(g, S / spp)
        worst = per_class(R, n, (rgb, g, S, Q), (want[0],) + want)
        print(f"{tag} n={n} spp={spp} lanes {lanes}: " + ", ".join(f"{c} {e:.2e}" for c, e in worst.items()))
        for c, e in worst.items():
            assert e <= ra.class_tol(c), c
    return g, S, Q


# 1 ------------------------------------------------- a scene without a BVH --
@pytest.mark.parametrize("case", CASES, ids=cid)
def test_render_rays_on_cornell(envs, case):
    """k_render_rays: mean, S and Q within 1e-12 of the oracle entry, boxed
    and plain handle; forced f64 the same bits; f32 output within 1e-6."""
    n, spp, rr_depth, s0 = case
    R, boxed, plain = envs("cornell")
    for r, tag in ((boxed, "cornell box"), (plain, "cornell plain")):
        got = check_against_oracle(R, r, n, spp, rr_depth, s0, PT_PATH_SINGLE, tag)
        f64 = r.render_rays(R.o[:n], R.d[:n], R.keys[:n], lanes_per_pixel=4, moments=True, force_f64=True,
                            **kw_of(spp, rr_depth, s0))
        assert all(same(x, y) for x, y in zip(got, f64))
    f32 = boxed.render_rays(R.o[:n], R.d[:n], R.keys[:n], out_f64=False, **kw_of(spp, rr_depth, s0))
    mean = moments(R.samples("cat", rr_depth, s0, spp)[:, :n])[0]
    assert f32.dtype == np.float32 and ra.rel(f32, mean) <= ra.TOL32


# 2 --------------------------------------------------- scenes with a BVH --
@pytest.mark.parametrize("case", CASES, ids=cid)
@pytest.mark.parametrize("name", BVH_SCENES)
def test_render_rays_through_the_wavefront_kernels(envs, name, case):
    """The wavefront route runs (last_launch), is within 1e-12 of the oracle
    entry and equals single_kernel=True bit for bit, boxed and plain; f32
    output within 1e-6."""
    n, spp, rr_depth, s0 = case
    R, boxed, plain = envs(name)
    for r, tag in ((boxed, name + " box"), (plain, name + " plain")):
        got = check_against_oracle(R, r, n, spp, rr_depth, s0, PT_PATH_WAVEFRONT, tag)
        sk = r.render_rays(R.o[:n], R.d[:n], R.keys[:n], lanes_per_pixel=4, moments=True, single_kernel=True,
                           **kw_of(spp, rr_depth, s0))
        assert r.last_launch()["path"] == PT_PATH_SINGLE
        assert all(same(x, y) for x, y in zip(got, sk))
    f32 = boxed.render_rays(R.o[:n], R.d[:n], R.keys[:n], out_f64=False, **kw_of(spp, rr_depth, s0))
    assert boxed.last_launch()["path"] == PT_PATH_WAVEFRONT
    mean = moments(R.samples("cat", rr_depth, s0, spp)[:, :n])[0]
    assert f32.dtype == np.float32 and ra.rel(f32, mean) <= ra.TOL32


@pytest.mark.parametrize("name", BVH_SCENES)
def test_a_record_does_not_depend_on_its_batch(envs, name):
    """All 257 records shuffled, and split into launches of 100 and 157: the
    same bits per record, every launch through the wavefront kernels."""
    R, r, _ = envs(name)
    kw = dict(kw_of(5, None, 0), moments=True, lanes_per_pixel=4)

    def go(sel):
        out = r.render_rays(R.o[sel], R.d[sel], R.keys[sel], **kw)
        assert r.last_launch()["path"] == PT_PATH_WAVEFRONT
        return out
    base = go(slice(None))
    perm = np.random.default_rng(3).permutation(ra.N_CAT)
    sh, one, two = go(perm), go(slice(0, 100)), go(slice(100, None))
    for x, y, z, w in zip(base, sh, one, two):
        assert same(np.ascontiguousarray(x[perm]), y) and same(x, np.concatenate([z, w]))


# 3 ------------------------------------------------------------- overflow --
@pytest.mark.parametrize("name", ("cornell",) + BVH_SCENES)
def test_overflow_class_is_zero(envs, name):
    """Lengths of 1e300 and 1e-300: the reference's value is 0 for every
    record (asserted), and so are mean, S and Q of every kernel."""
    R, boxed, plain = envs(name)
    o, d, k = R.overflow
    assert not R.samples("overflow", ns=5).any()
    for r in (boxed, plain):
        for more in ({}, dict(single_kernel=True), dict(force_f64=True)):
            for lanes in (1, 4):
                out = r.render_rays(o, d, k, moments=True, lanes_per_pixel=lanes, **kw_of(5, None, 0), **more)
                assert all(x.shape == (len(o), 3) and not x.any() for x in out), (name, more)


def test_unit_any_on_the_device():
    """The ray form's reflection of a caller's direction (pt_path.h unit_any,
    bounce<2>): v / sqrt(v.v) within 4 ulp for |v| from 1e-161 to 1e150 — a
    subnormal v.v is below rsqrt_d's range, where unit() is off by far more
    than the suite's 1e-12 (printed) — 0 where v.v overflows, and unit()'s own
    bits where v.v is normal."""
    gpu()
    lib = devcheck_lib.load()
    base = np.random.default_rng(5).normal(size=(64, 3))
    for scale in (1.0, 1e-30, 1e30, 1e150, 1e-150, 1e-155, 1e-158, 1e-160, 1e-161, 1e160):
        v = base * scale
        with np.errstate(over="ignore"):
            s = (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]
        want = v / np.sqrt(s)[:, None]
        got, plain = devcheck_lib.unit_any(lib, v)
        if np.isinf(s).all():
            assert not got.any() and not want.any()
            continue
        ulp = np.abs(got - want) / (np.abs(want) * 2.0 ** -52)
        miss = np.abs(plain - want).max()
        print(f"|v| ~ {scale:g}: unit_any within {ulp.max():.2f} ulp of v / sqrt(v.v); unit() off by {miss:.2e}")
        assert ulp.max() <= 4.0
        if s.min() >= 2.0 ** -1000:
            assert same(got, plain)
        else:
            assert s.max() < 2.0 ** -1022   # (subnormal sums of squares)


# 4 ------------------------------------------------------ the accumulator --
LOOK_W, LOOK_H = 10, 8
RULE = "r4-32-4"


def inside_batch(scene):
    """The inside look-at camera's 10 x 8 rays in list order as a
    rays_adaptive_ref.Batch whose samples are the oracle entry's."""
    o, d, k = cameras.look_at_rays(ra.INSIDE["eye"], ra.INSIDE["target"], fov_y=ra.INSIDE["fov_y"], W=LOOK_W, H=LOOK_H)
    eye = np.asarray(ra.INSIDE["eye"], dtype=np.float64)
    b = adaptive_ref.Batch(scene, records=(o, d, k, np.concatenate([eye, eye])),
                           source=lambda rr_depth, ns: oracle.radiance(b.pk, o, d, k, ra.BOUNCES, ra.SEED, ns))
    return b


@pytest.mark.parametrize("name", ["cornell", "mesh"])
def test_adaptive_run_on_the_inside_camera(envs, name):
    """A ray accumulator over the inside camera's rays: after every pass n is
    the simulation's on the oracle entry's samples and S, Q are within 1e-12;
    render_rays_adaptive's count map on the image-order records is the same
    run; tri of the features is oracle.intersect_objects on the same (o, d) and
    P within 1e-11 (tests/test_gpu_denoise.py's bar)."""
    R = envs(name)[0]
    b = inside_batch(R.scene)
    tol, floor, lo, hi, step = adaptive_ref.RULES[RULE]
    sim = b.simulate(RULE)
    samples = b.samples()
    hist = adaptive_sim.histogram(sim["n"])
    print(f"{name}: counts {hist}, {len(sim['passes'])} passes, margin {sim['margin']:.2e}")
    assert sim["margin"] >= adaptive_ref.MIN_MARGIN and len(hist) >= 3
    traj = adaptive_ref.trajectory(samples, RULE)
    p = make_params(b.n, 1, hi, ra.BOUNCES, ra.SEED)
    adapt = make_adapt(tol, hi, lo, step, floor)
    with Renderer(R.scene, ray_box=(b.box[:3], b.box[3:])) as r:
        with RayAccumulator(r, b.o, b.d, b.keys) as acc:
            for i, (n_active, added, n_after) in enumerate(traj):
                assert acc.select(adapt) == (n_active, added), f"pass {i + 1}"
                acc.render(p, adapt)
                m = acc.read(S=True, Q=True, n=True)
                assert np.array_equal(m["n"].reshape(-1), n_after), f"after pass {i + 1}"
                wS, wQ = adaptive_sim.moments_upto(samples, n_after)
                eS, eQ = ra.rel(m["S"].reshape(-1, 3), wS), ra.rel(m["Q"].reshape(-1, 3), wQ)
                assert eS <= ra.TOL and eQ <= ra.TOL, f"pass {i + 1}: {eS:.3e}, {eQ:.3e}"
            assert acc.select(adapt) == (0, 0)
            f = acc.features()
        tri, P = oracle.intersect_objects(b.pk, np.concatenate([b.o, b.d], axis=1))
        hit = tri >= 0
        assert hit.all()   # (a line from inside the room meets a wall)
        assert np.array_equal(f["tri"].reshape(-1), tri)
        dP = float(np.abs(f["P"].reshape(-1, 3) - P).max())
        print(f"{name}: features |P - oracle| = {dP:.3e}")
        assert dP <= 1e-11
        oi, di, ki = cameras.to_image_order(b.o, b.d, b.keys, LOOK_W, LOOK_H)
        res = r.render_rays_adaptive(oi, di, ki, (LOOK_H, LOOK_W), hi, ra.BOUNCES, tol, lo, step, floor, ra.SEED,
                                     moments=True)
        assert res.passes == sim["passes"]
        assert np.array_equal(cameras.from_image_order(res.counts, LOOK_W, LOOK_H), sim["n"])
        assert ra.rel(cameras.from_image_order(res.S, LOOK_W, LOOK_H), sim["S"]) <= ra.TOL
        assert ra.rel(cameras.from_image_order(res.Q, LOOK_W, LOOK_H), sim["Q"]) <= ra.TOL


# 5 ------------------------------------------------------------ the images --
@pytest.mark.parametrize("name", ["cornell", "mesh"])
def test_whole_small_images(envs, name):
    """10 x 8 images of look_at_rays from inside the room and of ortho_rays,
    placed by rays_to_image: every pixel within 1e-12 of the oracle entry's
    image."""
    R, _, plain = envs(name)
    lp = np.asarray(R.pk.tri_v, dtype=np.float64).reshape(-1, 3)[3 * R.pk.n_obj_tri:].mean(axis=0)
    views = {"look-at": cameras.look_at_rays(ra.INSIDE["eye"], ra.INSIDE["target"], fov_y=ra.INSIDE["fov_y"],
                                             W=LOOK_W, H=LOOK_H),
             "ortho": cameras.ortho_rays(ra.ORTHO["eye"], lp, width=9.0, W=LOOK_W, H=LOOK_H)}
    for view, (o, d, k) in views.items():
        want = oracle.radiance(R.pk, o, d, k, ra.BOUNCES, ra.SEED, 5).sum(axis=0) / 5
        lo, hi = cameras.rays_box(o)
        with Renderer(R.scene, ray_box=(lo, hi)) as r:
            got = r.render_rays(o, d, k, **kw_of(5, None, 0))
        img, ref = cameras.rays_to_image(got, LOOK_W, LOOK_H), cameras.rays_to_image(want, LOOK_W, LOOK_H)
        assert img.shape == (LOOK_H, LOOK_W, 3) and ref.any()
        print(f"{name} {view}: image against the oracle entry {ra.rel(img, ref):.3e}")
        assert ra.rel(img, ref) <= ra.TOL
        assert same(plain.render_rays(o, d, k, force_f64=True, **kw_of(5, None, 0)), got)


# 6 ----------------------------------------------------------- the goldens --
@pytest.mark.parametrize("fixture,scene,camera", ra.GOLDENS, ids=[g[0] for g in ra.GOLDENS])
def test_goldens_of_the_unmodified_reference(envs, fixture, scene, camera):
    """The unmodified reference's colours of caller-chosen rays, directly:
    within 1e-12, through the scene's own route and the single kernel."""
    g = np.load(os.path.join(GOLDEN, fixture))
    R, _, plain = envs(scene)
    spp, B, seed = int(g["spp"]), int(g["bounces"]), int(g["seed"])
    for more in ({}, dict(single_kernel=True)):
        got = plain.render_rays(g["o"], g["d"], g["keys"], spp=spp, bounces=B, seed=seed, **more)
        if not more:
            assert plain.last_launch()["path"] == (PT_PATH_SINGLE if scene == "cornell" else PT_PATH_WAVEFRONT)
        print(f"{fixture} {more}: {ra.rel(got, g['colors']):.3e}")
        assert ra.rel(got, g["colors"]) <= ra.TOL
