"""Radiance for caller-supplied rays on the host (pt_radiance, include/pt_capi.h;
pt_path.h rays_in_frame, rays_primary, RayHit with either sink): the lane code
compiled for the host (tests/hostcheck/pt_rays_host.cpp) against the oracle on
descriptors with the ray's origin as the eye (tests/rays_ref.py), the bitwise
equalities of the rule, the f32 filter's self-test from the box, the records of
scenes made by the older entries, the camera generators and the command line's
argument checks.  The GPU cases are tests/test_gpu_rays.py."""
import ctypes as C
import os

import numpy as np
import pytest

import hostlib
import rays_ref
from conftest import ROOT, hc_render

from pathtracerpython_amd import cameras, utils
from pathtracerpython_amd._abi import PT_FLAG_RR, make_lens, make_params, make_rays
from pathtracerpython_amd.pack import pack_scene

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)
TOL = 1e-12   # the project's f64 bar


@pytest.fixture(scope="module")
def rays_host(tmp_path_factory):
    """tests/hostcheck/pt_rays_host.cpp built by the hostcheck Makefile into a
    temporary directory."""
    lib = hostlib.build(tmp_path_factory.mktemp("rays_host"), "pt_rays_host")
    lib.hc_radiance.restype = C.c_int
    lib.hc_radiance.argtypes = [C.c_void_p, _dp, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_int32,
                                _dp, _dp, _dp, _ip]
    lib.hc_rays_record_hash.restype = C.c_int
    lib.hc_rays_record_hash.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]
    lib.hc_rays_records.restype = C.c_int
    lib.hc_rays_records.argtypes = [C.c_void_p, _dp, _ip, _dp]
    lib.hc_rays_in_frame.restype = C.c_int
    lib.hc_rays_in_frame.argtypes = [C.c_void_p, _dp, _dp, C.c_int64, _ip]
    lib.hc_rays_filter.restype = C.c_int
    lib.hc_rays_filter.argtypes = [C.c_void_p, _dp, C.c_int64, C.c_uint64, C.POINTER(C.c_int64)]
    lib.hc_render.restype = C.c_int
    lib.hc_render.argtypes = [C.c_void_p, C.c_void_p, C.c_int, _dp, C.c_void_p]
    return lib


@pytest.fixture(scope="module")
def benches(tmp_path_factory, cornell, mesh_golden):
    """name -> rays_ref.Bench, made at first use."""
    made = {}

    def get(name):
        if name not in made:
            made[name] = rays_ref.Bench(rays_ref.make_scene(name, tmp_path_factory.mktemp(name), cornell,
                                                            mesh_golden))
        return made[name]
    return get


def box_ptr(box):
    if box is None:
        return None
    return np.ascontiguousarray(box, dtype=np.float64).ctypes.data_as(_dp)


def host_radiance(lib, pk, box, o, d, keys, p, lanes=1, force64=False):
    """(sum, S, Q, route) of the host's ray kernel: [n, 3] f64 each, route [n]."""
    rec = make_rays(o, d, keys)
    n = rec.shape[0]
    a, S, Q = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, 3))
    route = np.zeros(n, dtype=np.int32)
    box = None if box is None else np.ascontiguousarray(box, dtype=np.float64)
    rc = lib.hc_radiance(C.addressof(pk.desc), box_ptr(box), C.c_void_p(rec.ctypes.data), n, C.addressof(p),
                         int(force64), int(lanes), a.ctypes.data_as(_dp), S.ctypes.data_as(_dp),
                         Q.ctypes.data_as(_dp), route.ctypes.data_as(_ip))
    assert rc == 0
    return a, S, Q, route


def ray_params(spp, bounces, rr_depth=None, sample_begin=0, seed=9):
    return make_params(1, 1, spp, bounces, seed, 0 if rr_depth is None else PT_FLAG_RR,
                       3 if rr_depth is None else rr_depth, sample_begin=sample_begin)


def test_abi_has_the_ray_entries():
    from pathtracerpython_amd import _native
    header = open(os.path.join(ROOT, "include", "pt_capi.h")).read()
    for name in ("pt_scene_create_rays", "pt_radiance_device", "pt_radiance"):
        assert f"int {name}(" in header and name in _native.EXPORTS
        if os.path.exists(_native.LIB_PATH):   # (a built tree: the library exports them)
            assert name.encode() + b"\0" in open(_native.LIB_PATH, "rb").read()
    assert "} pt_ray;" in header


# ------------------------------------------------------------ the oracle --
@pytest.mark.parametrize("boxed", [True, False], ids=["box", "plain"])
@pytest.mark.parametrize("case", rays_ref.PARITY_CASES, ids=rays_ref.case_id)
def test_oracle_parity(rays_host, benches, case, boxed):
    """Every record's mean, S and Q within 1e-12 of the oracle's per-sample
    colours on the descriptor with eye = o, none excluded; 1 and 4 lanes."""
    name, n, spp, bounces, rr_depth, s0 = case
    b = benches(name)
    esc, light, spec = rays_ref.first_hits(b.pk, b.o, b.d)
    print(f"{name}: batch of {len(b.o)}: {esc} escapes, {light} light hits, {spec} specular-material hits")
    assert esc >= 1 and light >= 1 and spec >= 1
    want = b.samples(n, bounces, rr_depth, s0, spp)
    p = ray_params(spp, bounces, rr_depth, s0)
    for lanes in (1, 4):
        if lanes > spp:
            continue
        a, S, Q, route = host_radiance(rays_host, b.pk, b.box if boxed else None, b.o[:n], b.d[:n], b.keys[:n],
                                       p, lanes)
        for what, got, ref in (("mean", a / spp, want.sum(axis=0) / spp), ("S", S, want.sum(axis=0)),
                               ("Q", Q, (want ** 2).sum(axis=0))):
            err = np.abs(got - ref)
            print(f"{rays_ref.case_id(case)} lanes {lanes}: |{what}| {err.max():.3e}")
            assert err.max() <= TOL, f"{what} off by {err.max():.3e} at record {int(err.max(axis=1).argmax())}"
        # the f64 route, as rays_primary reports it: the origins outside the frame the
        # scene was made for and no other (OFF_AXIS[1] is outside the plain frame too)
        if bounces > 0:
            assert np.array_equal(route, b.outside[:n].astype(np.int32))


def test_bounces_zero_is_zero(rays_host, benches):
    b = benches("cornell")
    a, S, Q, _ = host_radiance(rays_host, b.pk, None, b.o[:16], b.d[:16], b.keys[:16], ray_params(5, 0))
    assert not a.any() and not S.any() and not Q.any()


# ------------------------------------------------------ the frame's rays --
@pytest.mark.parametrize("W,H", [(12, 12), (7, 5)])
def test_frame_through_the_ray_entry_is_the_frame(rays_host, cornell, packed, W, H):
    """scene_camera_rays through the ray lane code is hc_render's frame, bit
    for bit (one lane per pixel: hc_render's)."""
    o, d, keys = cameras.scene_camera_rays(cornell, W, H)
    for spp, bounces in ((1, 2), (5, 3)):
        p = make_params(W, H, spp, bounces, 9)
        frame, _ = hc_render(rays_host, packed, p, count=False)
        a, _, _, route = host_radiance(rays_host, packed, None, o, d, keys, ray_params(spp, bounces))
        got = cameras.rays_to_image(a / spp, W, H)
        assert np.array_equal(got.view(np.uint64), np.ascontiguousarray(frame).view(np.uint64))
        assert not route.any()   # the eye is inside its own frame


def test_scene_camera_rays_are_make_rays_bit_for_bit(cornell):
    for W, H in ((12, 12), (7, 5), (1, 1), (3, 1)):
        o, d, keys = cameras.scene_camera_rays(cornell, W, H)
        x0, y0, x1, y1 = cornell.ortho
        ref = utils.make_rays(cornell.eye, utils.make_screen_pts(x0, y0, x1, y1, W, H))
        ro = np.array([np.asarray(r[0], dtype=np.float64) for r in ref])
        rd = np.array([np.asarray(r[1], dtype=np.float64) for r in ref])
        assert np.array_equal(o.view(np.uint64), ro.view(np.uint64))
        assert np.array_equal(d.view(np.uint64), rd.view(np.uint64))
        assert np.array_equal(keys, np.arange(W * H, dtype=np.uint32)) and keys.dtype == np.uint32


# ------------------------------------------------------------- the batch --
def test_a_record_does_not_depend_on_its_batch(rays_host, benches):
    """Shuffled, split in two, padded with other rays: the same bits per
    record; equal records give equal results."""
    b = benches("cornell")
    n = 65
    p = ray_params(8, 3)
    for lanes in (1, 4):
        base = host_radiance(rays_host, b.pk, b.box, b.o[:n], b.d[:n], b.keys[:n], p, lanes)[:3]
        perm = np.random.default_rng(3).permutation(n)
        sh = host_radiance(rays_host, b.pk, b.box, b.o[perm], b.d[perm], b.keys[perm], p, lanes)[:3]
        one = host_radiance(rays_host, b.pk, b.box, b.o[:20], b.d[:20], b.keys[:20], p, lanes)[:3]
        two = host_radiance(rays_host, b.pk, b.box, b.o[20:n], b.d[20:n], b.keys[20:n], p, lanes)[:3]
        pad = host_radiance(rays_host, b.pk, b.box, b.o[:n + 30][::-1], b.d[:n + 30][::-1], b.keys[:n + 30][::-1],
                            p, lanes)[:3]
        for x, y, z, w, v in zip(base, sh, one, two, pad):
            assert np.array_equal(x[perm], y)
            assert np.array_equal(x, np.concatenate([z, w]))
            assert np.array_equal(x, v[::-1][:n])
    twin = host_radiance(rays_host, b.pk, b.box, b.o[[4, 4, 9]], b.d[[4, 4, 9]], b.keys[[4, 4, 9]], p)
    assert np.array_equal(twin[0][0], twin[0][1]) and np.array_equal(twin[1][0], twin[1][1])
    # the lane count moves only the order of the sums
    a1 = host_radiance(rays_host, b.pk, b.box, b.o[:n], b.d[:n], b.keys[:n], p, 1)[0]
    a8 = host_radiance(rays_host, b.pk, b.box, b.o[:n], b.d[:n], b.keys[:n], p, 8)[0]
    assert np.abs(a1 - a8).max() / 8 <= TOL


# ---------------------------------------------------- f64 and the frames --
@pytest.mark.parametrize("name", ["cornell", "mesh"])
def test_forced_f64_is_the_hybrid_result_bit_for_bit(rays_host, benches, name):
    """Origins inside the box, outside it, and on a scene made without one; a
    ray with an out-of-frame origin took the f64 primary route."""
    b = benches(name)
    n = 64
    p = ray_params(5, 3)
    for box in (b.box, None):
        hyb = host_radiance(rays_host, b.pk, box, b.o[:n], b.d[:n], b.keys[:n], p)
        f64 = host_radiance(rays_host, b.pk, box, b.o[:n], b.d[:n], b.keys[:n], p, force64=True)
        for x, y in zip(hyb[:3], f64[:3]):
            assert np.array_equal(x.view(np.uint64), y.view(np.uint64))
        route = hyb[3]
        assert route[b.outside[:n]].all() and b.outside[:n].any()
        assert not route[~b.outside[:n]].any()
        assert f64[3].all()


def test_the_frame_admits_the_box_and_nothing_far_from_it(rays_host, benches):
    b = benches("cornell")
    corners = np.array([[b.box[3 * (c & 1)], b.box[1 + 3 * ((c >> 1) & 1)], b.box[2 + 3 * ((c >> 2) & 1)]]
                        for c in range(8)])
    eye = np.array([[float(v) for v in b.pk.eye]])
    X = np.zeros(4)
    same = np.zeros(4, dtype=np.int32)
    assert rays_host.hc_rays_records(C.addressof(b.pk.desc), box_ptr(b.box), same.ctypes.data_as(_ip),
                                     X.ctypes.data_as(_dp)) == 0
    far = X[:3] + np.array([[X[3] * 1.001, 0, 0], [0, -X[3] * 1.001, 0], [0, 0, X[3] * 1.001], [np.nan, 0, 0],
                            [np.inf, 0, 0]])
    pts = np.ascontiguousarray(np.concatenate([corners, eye, b.o[~b.outside], far]))
    got = np.zeros(len(pts), dtype=np.int32)
    assert rays_host.hc_rays_in_frame(C.addressof(b.pk.desc), box_ptr(b.box), pts.ctypes.data_as(_dp), len(pts),
                                      got.ctypes.data_as(_ip)) == 0
    assert got[:-5].all() and not got[-5:].any()
    # a plain scene: the cube about the box of the triangles and the eye
    got = np.zeros(2, dtype=np.int32)
    pts = np.ascontiguousarray(np.array(rays_ref.OFF_AXIS))
    assert rays_host.hc_rays_in_frame(C.addressof(b.pk.desc), None, pts.ctypes.data_as(_dp), 2,
                                      got.ctypes.data_as(_ip)) == 0
    assert list(got) == [1, 0]


@pytest.mark.parametrize("name", ["cornell", "mesh"])
def test_filter_selftest_from_the_box(rays_host, benches, name):
    """Random lines from random points of a box well beyond the scene's own
    frame: no wrong certain verdict, every origin admitted."""
    b = benches(name)
    box = np.array([-9.0, -7.0, -30.0, 11.0, 8.0, 14.0])
    out = (C.c_int64 * 4)()
    assert rays_host.hc_rays_filter(C.addressof(b.pk.desc), box_ptr(box), 4000, 11, out) == 0
    wrong, amb, tests, outside = list(out)
    print(f"{name}: {tests} tests from the box, {amb} ambiguous, {wrong} wrong, {outside} origins refused")
    assert wrong == 0 and outside == 0 and tests > 100000 and amb < tests // 10


# The parent commit's FNV-1a of {unit, unit_eye, bunit, kd} of the scene
# made by pt_scene_create and by pt_scene_create_lens with (0.25, -24)
PARENT_RECORDS = {
    ("cornell", False): (0xc77371ef103e153f, 0xa546f740b11762fb, 0xcbf29ce484222325, 0xaa3ab17d19a80c20),
    ("cornell", True): (0xc77371ef103e153f, 0xa546f740b11762fb, 0xcbf29ce484222325, 0x64535ea215026237),
    ("mesh", False): (0x28b9efde1f3428b1, 0x2e788820febd3ab5, 0xb97d4b4f4b5aeae5, 0x4c00765d19234114),
    ("mesh", True): (0x28b9efde1f3428b1, 0x2e788820febd3ab5, 0xb97d4b4f4b5aeae5, 0xade840fa266b26f3),
}


@pytest.mark.parametrize("name", ["cornell", "mesh"])
def test_scenes_from_the_old_entries_keep_their_records(rays_host, benches, name):
    b = benches(name)
    for lens in (False, True):
        L = make_lens((0.25, -24.0)) if lens else None
        out = (C.c_uint64 * 4)()
        assert rays_host.hc_rays_record_hash(C.addressof(b.pk.desc), C.addressof(L) if L else None, out) == 0
        assert tuple(out) == PARENT_RECORDS[(name, lens)]
    same, X = np.zeros(4, dtype=np.int32), np.zeros(4)
    # no box: the scene of pt_scene_create; a box inside the frame changes nothing either
    for box in (None, [0, 0, 0, 1, 1, 1]):
        assert rays_host.hc_rays_records(C.addressof(b.pk.desc), box_ptr(box), same.ctypes.data_as(_ip),
                                         X.ctypes.data_as(_dp)) == 0
        assert same.all()
    # a box beyond the eye moves the frame: unit_eye's bounds and kd change, the surface frame's units do not
    assert rays_host.hc_rays_records(C.addressof(b.pk.desc), box_ptr([0, 0, 0, 1, 1, 40]),
                                     same.ctypes.data_as(_ip), X.ctypes.data_as(_dp)) == 0
    assert same[0] and not same[1] and not same[3]
    for bad in ([0, 0, 0, 1, 1, np.nan], [0, 0, 2, 1, 1, 1], [0, 0, 0, np.inf, 1, 1]):
        assert rays_host.hc_rays_records(C.addressof(b.pk.desc), box_ptr(bad), same.ctypes.data_as(_ip),
                                         X.ctypes.data_as(_dp)) == -1


# ------------------------------------------------------------ the cameras --
def test_look_at_rays():
    eye, target, up = (1.0, 2.0, 9.0), (0.5, -1.0, -20.0), (0.0, 1.0, 0.0)
    for W, H in ((9, 7), (8, 8), (1, 1)):
        o, d, keys = cameras.look_at_rays(eye, target, up, 35.0, W, H)
        assert o.shape == d.shape == (W * H, 3) and np.array_equal(o, np.broadcast_to(eye, (W * H, 3)))
        assert np.abs(np.linalg.norm(d, axis=1) - 1.0).max() <= 1e-15
        assert np.array_equal(keys, np.arange(W * H, dtype=np.uint32))
    o, d, _ = cameras.look_at_rays(eye, target, up, 35.0, 9, 7)
    f = np.subtract(target, eye)
    f /= np.linalg.norm(f)
    img = cameras.rays_to_image(d, 9, 7)               # (H, W, 3), top row first
    assert np.abs(img[3, 4] - f).max() <= 1e-15        # the centre ray goes through the target
    # the up vector: the image's top is on up's side, its right is f x up
    assert np.dot(img[0, 4] - img[6, 4], up) > 0
    assert np.dot(img[3, 8] - img[3, 0], np.cross(f, up)) > 0
    assert abs(np.dot(img[0, 4] - img[6, 4], np.cross(f, up))) <= 1e-15
    # the field of view: the top and bottom pixel centres span fov_y * (H - 1)/H in tangent
    t = np.tan(np.radians(35.0) / 2) * 6 / 7
    top = img[0, 4] / np.dot(img[0, 4], f)
    assert abs(np.linalg.norm(top - f) - t) <= 1e-14
    with pytest.raises(ValueError):
        cameras.look_at_rays(eye, eye)
    with pytest.raises(ValueError):
        cameras.look_at_rays((0, 0, 0), (0, 1, 0), (0, 2, 0))


def test_ortho_rays_are_parallel():
    o, d, keys = cameras.ortho_rays((0.0, 0.0, 5.0), (0.0, 0.0, -20.0), width=6.0, W=6, H=3)
    assert np.array_equal(d, np.broadcast_to([0.0, 0.0, -1.0], (18, 3)))
    img = cameras.rays_to_image(o, 6, 3)
    assert np.allclose(img[:, :, 2], 5.0) and np.allclose(img[1, :, 1], 0.0)
    assert np.allclose(img[0, :, 0], [-2.5, -1.5, -0.5, 0.5, 1.5, 2.5])   # right is f x up = +x
    assert np.allclose(img[0, 0, 1], 1.0) and np.allclose(img[2, 0, 1], -1.0)   # square pixels: height 3
    lo, hi = cameras.rays_box(o)
    assert np.allclose(lo, [-2.5, -1.0, 5.0]) and np.allclose(hi, [2.5, 1.0, 5.0])


def test_rays_to_image_is_the_list_order_placement():
    from pathtracerpython_amd.render import from_list_order
    v = np.arange(5 * 3 * 3, dtype=np.float64).reshape(15, 3)
    assert np.array_equal(cameras.rays_to_image(v, 5, 3), from_list_order(v, 5, 3))


def test_make_rays_records():
    rec = make_rays([[1, 2, 3], [4, 5, 6]], [[0, 0, -1], [0, 1, 0]])
    assert rec.dtype.itemsize == 56 and list(rec["key"]) == [0, 1] and not rec["reserved"].any()
    raw = np.frombuffer(rec.tobytes(), dtype=np.float64).reshape(2, 7)
    assert np.array_equal(raw[:, :6], [[1, 2, 3, 0, 0, -1], [4, 5, 6, 0, 1, 0]])
    with pytest.raises(ValueError):
        make_rays([[0, 0, 0]], [[0, 0, 1]], keys=[1 << 32])
    with pytest.raises(ValueError):
        make_rays([[0, 0, 0]], [[0, 0, 1], [0, 0, 1]])


# ------------------------------------------------------- the command line --
@pytest.mark.parametrize("extra", [["--aa"], ["--aperture", "0.2", "--focus-z", "-20"], ["--noise", "0.05", "-r", "16"],
                                   ["--denoise", "-r", "4"], ["--devices", "2"], ["--local-devices", "1"],
                                   ["--chunk-spp", "2", "-r", "4"], ["--fov", "180"]])
def test_cli_refuses_what_look_at_does_not_take(extra):
    from pathtracerpython_amd import main as cli
    args = cli.setup(["scene.sdl", "--look-at", "1", "2", "9", "0", "0", "-20"] + extra)
    with pytest.raises(SystemExit) as e:
        cli.check_args(args)
    assert "--look-at" in str(e.value) or "--fov" in str(e.value)


def test_cli_refuses_up_and_fov_without_look_at():
    from pathtracerpython_amd import main as cli
    for extra in (["--up", "0", "0", "1"], ["--fov", "50"]):
        with pytest.raises(SystemExit, match="--look-at"):
            cli.check_args(cli.setup(["scene.sdl"] + extra))
    args = cli.setup(["scene.sdl", "--look-at", "1", "2", "9", "0", "0", "-20"])
    cli.check_args(args)
    assert list(args.up) == [0.0, 1.0, 0.0] and args.fov == 40.0


def test_cli_accepts_look_at_with_its_own_flags():
    from pathtracerpython_amd import main as cli
    args = cli.setup(["scene.sdl", "--look-at", "1", "2", "9", "0", "0", "-20", "--up", "0", "0", "1", "--fov", "50",
                      "-r", "4", "-b", "2", "--rr", "--seed", "3", "--size", "8", "6", "--out", "x.png",
                      "--save-raw", "x.npy"])
    cli.check_args(args)
    assert args.look_at == [1.0, 2.0, 9.0, 0.0, 0.0, -20.0] and list(args.up) == [0.0, 0.0, 1.0]
