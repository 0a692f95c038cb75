"""The thin-lens camera on the host (PT_FLAG_LENS, include/pt_capi.h; pt_path.h
lens_point, lens_window, lens_dir, LensRay with either sink): the rule's
helpers against their numpy restatement, the sample loop compiled for the host
against the oracle on shifted eyes and screen windows (tests/lens_ref.py), the
bitwise equalities of the rule, the f32 filter's self-test from the lens disc,
the stop rule on lens frames, the checkpoint keys and the argument checks.
The GPU cases are tests/test_gpu_lens.py."""
import ctypes as C
import os

import numpy as np
import pytest

import hostlib
import aa_ref
import lens_ref
from adaptive_sim import histogram, simulate
from conftest import ROOT

from pathtracerpython_amd import adaptive, progressive
from pathtracerpython_amd._abi import PT_FLAG_AA, PT_FLAG_LENS, PT_FLAG_RR, make_lens, make_params
from pathtracerpython_amd.pack import pack_scene

_dp = C.POINTER(C.c_double)
_up = C.POINTER(C.c_uint32)

A, B = lens_ref.CASE_A, lens_ref.CASE_B
TOL = 1e-12   # the project's f64 bar


def flags_of(case, extra=0):
    return PT_FLAG_LENS | (PT_FLAG_AA if case["aa"] else 0) | extra


def lens_of(case):
    return make_lens((case["R"], case["zf"]))


@pytest.fixture(scope="module")
def lens_host(tmp_path_factory):
    """tests/hostcheck/pt_lens_host.cpp built by the hostcheck Makefile into a
    temporary directory."""
    lib = hostlib.build(tmp_path_factory.mktemp("lens_host"), "pt_lens_host")
    lib.hc_lens_point.restype = None
    lib.hc_lens_point.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_int32, C.c_double, _dp]
    lib.hc_lens_dir.restype = C.c_int
    lib.hc_lens_dir.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                C.c_double, C.c_double, C.c_double, C.c_double, _dp, _dp, _dp]
    lib.hc_lens_check.restype = C.c_int
    lib.hc_lens_check.argtypes = [C.c_void_p, C.c_void_p]
    lib.hc_lens_records.restype = C.c_int
    lib.hc_lens_records.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int32), _dp]
    lib.hc_render_lens.restype = C.c_int
    lib.hc_render_lens.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int32, _dp, _dp, _dp]
    lib.hc_accum_lens.restype = C.c_int
    lib.hc_accum_lens.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_uint32,
                                  C.c_uint32, C.c_uint32, _dp, _dp, _up]
    lib.hc_lens_filter.restype = C.c_int
    lib.hc_lens_filter.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_uint64, C.POINTER(C.c_int64)]
    return lib


def host_lens(lib, pk, lens, p, lanes=1, force64=False):
    """(sum, S, Q) [H, W, 3] of the host's sample loop; lens: a PtLens or None."""
    H, W = p.height, p.width
    a, S, Q = np.zeros((H, W, 3)), np.zeros((H, W, 3)), np.zeros((H, W, 3))
    rc = lib.hc_render_lens(C.addressof(pk.desc), C.addressof(lens) if lens is not None else None,
                            C.addressof(p), int(force64), int(lanes), a.ctypes.data_as(_dp),
                            S.ctypes.data_as(_dp), Q.ctypes.data_as(_dp))
    assert rc == 0
    return a, S, Q


def reference(scene, case, W=12, H=12, n=8, want_light=True):
    """Per-sample frames of a case in list order, with the restart loop's
    branches asserted before anything is compared."""
    c = lens_ref.lens_samples(scene, W, H, 3, 9, n, **case)
    me, ml, ae = lens_ref.coverage(c, pack_scene(scene).light_rgb)
    print(f"coverage {W}x{H} {case}: mixed-escape {me}, mixed-light {ml}, all-escape {ae}")
    assert me >= 1 and ae >= 1 and (ml >= 1 or not want_light)
    return c


@pytest.fixture(scope="module")
def refA(cornell):
    return lens_ref.to_image(reference(cornell, A), 12, 12)


@pytest.fixture(scope="module")
def refB(cornell):
    return lens_ref.to_image(reference(cornell, B, want_light=False), 12, 12)


# ------------------------------------------------------------ the helpers --
@pytest.mark.parametrize("W,H", [(7, 5), (1, 1), (3, 1)])
def test_window_and_direction_are_numpy_bit_for_bit(lens_host, cornell, W, H):
    """Steps 4-5 given (jx, jy, lx, ly)."""
    pk = pack_scene(cornell)
    for case in (A, B, dict(R=2.0, zf=0.0, aa=True)):
        L = lens_of(case)
        kap = lens_ref.kappa(pk.eye[2], case["zf"])
        for ix in range(W):
            for iy in range(H):
                k = ix * H + iy
                for s in (0, 1, 5, 1000003):
                    jx, jy = lens_ref.jitter(9, k, s, case["aa"])
                    lx, ly, _ = lens_ref.lens_point(9, k, s, case["R"])
                    win, d0, eye = np.zeros(4), np.zeros(3), np.zeros(3)
                    rc = lens_host.hc_lens_dir(C.addressof(pk.desc), C.addressof(L), W, H, ix, iy, float(jx),
                                               float(jy), float(lx), float(ly), win.ctypes.data_as(_dp),
                                               d0.ctypes.data_as(_dp), eye.ctypes.data_as(_dp))
                    assert rc == 0
                    want_d, want_w, want_e = lens_ref.direction(pk.ortho, pk.eye, W, H, ix, iy, jx, jy, lx, ly, kap)
                    assert np.array_equal(win.view(np.uint64), want_w.view(np.uint64))
                    assert np.array_equal(d0.view(np.uint64), want_d.view(np.uint64))
                    assert np.array_equal(eye.view(np.uint64), want_e.view(np.uint64))
                    if case["zf"] == 0.0 and not case["aa"]:
                        assert np.array_equal(win, pk.ortho)


def test_focus_on_the_screen_moves_only_the_eye(lens_host, packed):
    """zf = 0: kappa = 0, the window is the jittered one whatever the lens point."""
    L = make_lens((2.0, 0.0))
    win, d0, eye = np.zeros(4), np.zeros(3), np.zeros(3)
    assert lens_host.hc_lens_dir(C.addressof(packed.desc), C.addressof(L), 7, 5, 3, 2, 0.0, 0.0, 1.25, -0.5,
                                 win.ctypes.data_as(_dp), d0.ctypes.data_as(_dp), eye.ctypes.data_as(_dp)) == 0
    assert np.array_equal(win, packed.ortho)
    assert eye[0] == packed.eye[0] + 1.25 and eye[1] == packed.eye[1] - 0.5 and eye[2] == packed.eye[2]


@pytest.mark.parametrize("R", [0.25, 0.5, 2.0])
def test_lens_point_against_numpy(lens_host, R):
    """The lens point within R*2^-48 per coordinate of numpy's (sqrt_d <= 3 ulp,
    sincos_small <= 2^-52 absolute, one product rounding); r <= R always; the
    jitter is PT_FLAG_AA's, or zero without it."""
    worst = 0.0
    for k in range(40):
        for s in (0, 1, 7, 1000003):
            for aa in (0, 1):
                o = np.zeros(5)
                lens_host.hc_lens_point(9, k, s, aa, R, o.ctypes.data_as(_dp))
                lx, ly, r = lens_ref.lens_point(9, k, s, R)
                worst = max(worst, abs(o[2] - lx), abs(o[3] - ly))
                assert abs(o[2] - lx) <= R * 2.0 ** -48 and abs(o[3] - ly) <= R * 2.0 ** -48
                assert 0.0 <= o[4] <= R and abs(o[4] - r) <= R * 2.0 ** -49
                jx, jy = aa_ref.jitter(9, k, s) if aa else (0.0, 0.0)
                assert o[0] == jx and o[1] == jy
    print(f"R {R}: lens point off numpy's by at most {worst:.3e} (bound {R * 2.0 ** -48:.3e})")
    o = np.zeros(5)
    lens_host.hc_lens_point(9, 3, 4, 1, 0.0, o.ctypes.data_as(_dp))
    assert o[2] == 0.0 and o[3] == 0.0 and o[4] == 0.0     # R = 0: the pinhole


def test_lens_point_is_keyed_by_seed_pixel_and_sample():
    a = lens_ref.lens_point(9, 3, 4, 0.5)
    assert a == lens_ref.lens_point(9, 3, 4, 0.5)
    assert a != lens_ref.lens_point(10, 3, 4, 0.5) and a != lens_ref.lens_point(9, 4, 4, 0.5)
    assert a != lens_ref.lens_point(9, 3, 5, 0.5) and a != lens_ref.lens_point(9 + (1 << 32), 3, 4, 0.5)


# --------------------------------------------------------- the sample loop --
def check_against(a, S, Q, want, what):
    """Per-pixel sums of per-sample colours within the bar; names the worst
    pixel when it is missed."""
    for name, got, ref in (("sum", a, want.sum(axis=0)), ("S", S, want.sum(axis=0)),
                           ("Q", Q, (want ** 2).sum(axis=0))):
        d = np.abs(got - ref)
        row, col, ch = np.unravel_index(int(d.argmax()), d.shape)
        print(f"{what}: |{name}| {d.max():.3e}")
        assert d.max() <= TOL, f"{what}: {name} off by {d.max():.3e} at image row {row}, column {col}, channel {ch}"


@pytest.mark.parametrize("lanes", [1, 4, 8])
def test_host_sample_loop_matches_the_oracle_case_a(lens_host, cornell, refA, lanes):
    pk = pack_scene(cornell)
    a, S, Q = host_lens(lens_host, pk, lens_of(A), make_params(12, 12, 8, 3, 9, flags_of(A)), lanes)
    check_against(a, S, Q, refA, f"A, {lanes} lanes")


@pytest.mark.parametrize("lanes", [1, 4, 8])
def test_host_sample_loop_matches_the_oracle_case_b(lens_host, cornell, refB, lanes):
    pk = pack_scene(cornell)
    a, S, Q = host_lens(lens_host, pk, lens_of(B), make_params(12, 12, 8, 3, 9, flags_of(B)), lanes)
    check_against(a, S, Q, refB, f"B, {lanes} lanes")


def test_each_sample_matches_the_oracle(lens_host, cornell, refA):
    """One sample at a time (sample_begin = s, spp 1): a miss names pixel and sample."""
    pk = pack_scene(cornell)
    L = lens_of(A)
    for s in range(8):
        a, _, _ = host_lens(lens_host, pk, L, make_params(12, 12, 1, 3, 9, flags_of(A), sample_begin=s))
        d = np.abs(a - refA[s])
        row, col, _ = np.unravel_index(int(d.argmax()), d.shape)
        assert d.max() <= TOL, f"sample {s}, image row {row}, column {col}: {d.max():.3e}"


def test_sample_ranges_rr_and_no_bounces(lens_host, cornell, refA):
    pk = pack_scene(cornell)
    L = lens_of(A)
    a, _, _ = host_lens(lens_host, pk, L, make_params(12, 12, 3, 3, 9, flags_of(A), sample_begin=5))
    assert np.abs(a - refA[5:8].sum(axis=0)).max() <= TOL
    a, S, _ = host_lens(lens_host, pk, L, make_params(12, 12, 8, 0, 9, flags_of(A)))
    assert not a.any() and not S.any()
    c = lens_ref.to_image(lens_ref.lens_samples(cornell, 8, 8, 4, 9, 4, flags=PT_FLAG_RR, rr_depth=1, **A), 8, 8)
    a, _, _ = host_lens(lens_host, pk, L, make_params(8, 8, 4, 4, 9, flags_of(A, PT_FLAG_RR), 1))
    assert np.abs(a - c.sum(axis=0)).max() <= TOL


def test_bvh_scene_matches_the_oracle(lens_host, mesh_golden):
    sc, _ = mesh_golden
    want = lens_ref.to_image(lens_ref.lens_samples(sc, 12, 12, 3, 5, 2, **A), 12, 12)
    a, S, Q = host_lens(lens_host, pack_scene(sc), lens_of(A), make_params(12, 12, 2, 3, 5, flags_of(A)))
    check_against(a, S, Q, want, "mesh scene")


# ------------------------------------------------------ bitwise equalities --
def same3(x, y):
    return all(np.array_equal(np.ascontiguousarray(u).view(np.uint64), np.ascontiguousarray(v).view(np.uint64))
               for u, v in zip(x, y))


def test_radius_zero_is_the_pinhole(lens_host, cornell):
    pk = pack_scene(cornell)
    L0 = make_lens((0.0, -24.0))
    aa = host_lens(lens_host, pk, None, make_params(12, 12, 8, 3, 9, PT_FLAG_AA), 4)
    assert same3(host_lens(lens_host, pk, L0, make_params(12, 12, 8, 3, 9, PT_FLAG_LENS | PT_FLAG_AA), 4), aa)
    plain = host_lens(lens_host, pk, None, make_params(12, 12, 8, 3, 9), 4)
    assert same3(host_lens(lens_host, pk, L0, make_params(12, 12, 8, 3, 9, PT_FLAG_LENS), 4), plain)
    assert plain[0].any() and not same3(aa, plain)


def test_a_lens_scene_without_the_flag_is_the_plain_scene(lens_host, cornell, mesh_golden):
    """Another "all" frame (centre, half extent, error bounds), the same frames."""
    for sc, p in ((cornell, make_params(12, 12, 8, 3, 9)), (cornell, make_params(12, 12, 8, 3, 9, PT_FLAG_AA)),
                  (mesh_golden[0], make_params(12, 12, 2, 3, 5))):
        pk = pack_scene(sc)
        plain = host_lens(lens_host, pk, None, p)
        for R in (0.5, 2.0):
            assert same3(host_lens(lens_host, pk, make_lens((R, -24.0)), p), plain)


def test_hybrid_equals_forced_f64(lens_host, cornell, mesh_golden):
    """Origins on the disc are new ground for the eye-frame filter records."""
    for sc, case, p in ((cornell, A, make_params(12, 12, 8, 3, 9, flags_of(A))),
                        (cornell, B, make_params(12, 12, 8, 3, 9, flags_of(B))),
                        (mesh_golden[0], A, make_params(12, 12, 2, 3, 5, flags_of(A))),
                        (mesh_golden[0], B, make_params(12, 12, 2, 3, 5, flags_of(B)))):
        pk = pack_scene(sc)
        got = host_lens(lens_host, pk, lens_of(case), p)
        assert got[0].any() and same3(got, host_lens(lens_host, pk, lens_of(case), p, force64=True))


# ----------------------------------------------------- the prepared scene --
def test_records_without_a_lens_are_byte_identical(lens_host, packed, mesh_golden):
    for pk in (packed, pack_scene(mesh_golden[0])):
        out, same, X = (C.c_int64 * 4)(), (C.c_int32 * 4)(), np.zeros(2)
        assert lens_host.hc_lens_records(C.addressof(pk.desc), None, out, same, X.ctypes.data_as(_dp)) == 0
        assert list(same) == [1, 1, 1, 1] and out[1] > 0 and out[3] == 16 * 8
        eh0 = X[1]
        # a disc wider than the room: the surface frame is untouched, the "all"
        # frame's bounds grow with its box, and kd knows the lens
        L = make_lens((50.0, -24.0))
        assert lens_host.hc_lens_records(C.addressof(pk.desc), C.addressof(L), out, same,
                                         X.ctypes.data_as(_dp)) == 0
        assert same[0] == 1 and same[1] == 0 and same[3] == 0
        assert X[1] > eh0
        # R = 0: the frame is the pinhole's, only kd differs (zf, kappa)
        L = make_lens((0.0, -24.0))
        assert lens_host.hc_lens_records(C.addressof(pk.desc), C.addressof(L), out, same,
                                         X.ctypes.data_as(_dp)) == 0
        assert list(same) == [1, 1, 1, 0]


@pytest.mark.parametrize("R", [0.5, 2.0])
def test_filter_selftest_from_the_lens(lens_host, packed, mesh_golden, R):
    """filter_eval.h's forms over unit_eye from origins on the disc (centre,
    rim, the four axis points): no wrong certain verdict against eval64."""
    for pk, n in ((packed, 3000), (pack_scene(mesh_golden[0]), 600)):
        out = (C.c_int64 * 3)()
        L = make_lens((R, -24.0))
        assert lens_host.hc_lens_filter(C.addressof(pk.desc), C.addressof(L), n, 11, out) == 0
        print(f"R {R}: {out[2]} tests, {out[1]} ambiguous ({out[1] / out[2]:.3%}), {out[0]} wrong")
        assert out[2] > 0 and out[0] == 0


def test_lens_validation(lens_host, packed, cornell):
    ez = float(packed.eye[2])
    assert ez > 0                                        # (the Cornell eye: in front of the screen)
    ok = [(0.0, -24.0), (0.25, -24.0), (2.0, 0.0), (1.0, ez / 2)]
    bad = [(-0.1, -24.0), (float("nan"), -24.0), (0.5, float("inf")), (float("inf"), -24.0),
           (0.5, ez), (0.5, 2 * ez), (0.5, float("nan"))]
    for R, zf in ok:
        L = make_lens((R, zf))
        assert lens_host.hc_lens_check(C.addressof(packed.desc), C.addressof(L)) == 0, (R, zf)
    for R, zf in bad:
        L = make_lens((R, zf))
        assert lens_host.hc_lens_check(C.addressof(packed.desc), C.addressof(L)) == -1, (R, zf)
    pk = pack_scene(cornell)
    pk.desc.eye[2] = 0.0                                 # ez = 0: no lens
    L = make_lens((0.5, -24.0))
    assert lens_host.hc_lens_check(C.addressof(pk.desc), C.addressof(L)) == -1
    assert lens_host.hc_lens_check(C.addressof(pk.desc), None) == 0


# --------------------------------------------------------- the adaptive rule --
FLOOR = 1e-3
STOP_TOL = 0.05


@pytest.fixture(scope="module")
def ref16(cornell):
    """Input A at 16x16, 32 samples (the rule (3, 17, 5) reads the first 17)."""
    return lens_ref.to_image(lens_ref.lens_samples(cornell, 16, 16, 3, 9, 32, **A), 16, 16)


@pytest.mark.parametrize("rule", [(4, 32, 4), (3, 17, 5)])
def test_adaptive_rule_on_lens_frames(lens_host, cornell, ref16, rule):
    mn, mx, st = rule
    sim = simulate(ref16[:mx], STOP_TOL, FLOOR, mn, mx, st)
    print(f"rule {rule}: margin {sim['margin']:.3e}, counts {histogram(sim['n'])}")
    assert sim["margin"] >= 1e-9   # sums that differ by 1e-12 cannot flip a count
    assert len(histogram(sim["n"])) >= 3
    pk = pack_scene(cornell)
    L = lens_of(A)
    S, Q = np.zeros((16, 16, 3)), np.zeros((16, 16, 3))
    n = np.zeros((16, 16), dtype=np.uint32)
    p = make_params(16, 16, mx, 3, 9, flags_of(A))
    rc = lens_host.hc_accum_lens(C.addressof(pk.desc), C.addressof(L), C.addressof(p), STOP_TOL, FLOOR, mn, mx,
                                 st, S.ctypes.data_as(_dp), Q.ctypes.data_as(_dp), n.ctypes.data_as(_up))
    assert rc == len(sim["passes"])
    assert np.array_equal(n, sim["n"])
    assert np.abs(S - sim["S"]).max() <= TOL and np.abs(Q - sim["Q"]).max() <= TOL


# ------------------------------------------------------------- checkpoints --
def test_checkpoint_keys(packed, tmp_path):
    old = {"scene": progressive.scene_fingerprint(packed), "width": 8, "height": 8, "spp": 4,
           "bounces": 2, "seed": 9, "rr": False, "rr_depth": 3, "chunk_spp": 2}
    off = progressive.run_key(packed, 8, 8, 4, 2, 9, False, 3, 2)
    on = progressive.run_key(packed, 8, 8, 4, 2, 9, False, 3, 2, lens=(0.25, -24))
    both = progressive.run_key(packed, 8, 8, 4, 2, 9, False, 3, 2, aa=True, lens=(0.25, -24))
    assert off == old and "lens" not in off         # an old key dict compares equal
    assert on == {**old, "lens": [0.25, -24.0]} and both == {**on, "aa": True}
    ck = progressive.Checkpoint(tmp_path / "p.npz")
    ck.save(on, np.zeros((8, 8, 3)), 2)
    assert ck.load(on)[1] == 2
    for other in (off, both, progressive.run_key(packed, 8, 8, 4, 2, 9, False, 3, 2, lens=(0.25, -32)),
                  progressive.run_key(packed, 8, 8, 4, 2, 9, False, 3, 2, lens=(0.5, -24))):
        with pytest.raises(ValueError, match="another render"):
            ck.load(other)
    ck.save(off, np.zeros((8, 8, 3)), 2)
    with pytest.raises(ValueError, match="another render"):
        ck.load(on)                                  # a pinhole file with a lens

    olda = {"scene": progressive.scene_fingerprint(packed), "width": 8, "height": 8,
            "bounces": 2, "seed": 9, "rr": False, "rr_depth": 3, "lanes_per_pixel": 4}
    offa = adaptive.accum_key(packed, 8, 8, 2, 9, False, 3, 4)
    ona = adaptive.accum_key(packed, 8, 8, 2, 9, False, 3, 4, lens=(0.25, -24))
    assert offa == olda and ona == {**olda, "lens": [0.25, -24.0]}
    ca = adaptive.AccumCheckpoint(tmp_path / "a.npz")
    z = (np.zeros((8, 8, 3)), np.zeros((8, 8, 3)), np.zeros((8, 8), dtype=np.uint32))
    ca.save(ona, {"tol": 0.05}, *z, [(64, 256)])
    assert ca.load(ona)["passes"] == [(64, 256)]
    with pytest.raises(ValueError, match="another render"):
        ca.load(offa)
    ca.save(offa, {"tol": 0.05}, *z, [])
    with pytest.raises(ValueError, match="another render"):
        ca.load(ona)


def test_lens_argument_rule():
    """lens=None means "on iff the renderer has a lens"; a renderer without
    one cannot be asked for it."""
    from pathtracerpython_amd.render import Renderer

    class R:
        lens_on = Renderer.lens_on
    r = R()
    r.lens = None
    assert r.lens_on() is False and r.lens_on(False) is False and progressive.lens_of(r) is None
    with pytest.raises(ValueError, match="created with a lens"):
        r.lens_on(True)
    r.lens = (0.25, -24.0)
    assert r.lens_on() is True and r.lens_on(True) is True and r.lens_on(False) is False
    assert progressive.lens_of(r) == (0.25, -24.0) and progressive.lens_of(r, False) is None
    assert progressive.lens_of(object()) is None          # a renderer that knows no lens


def test_flag_and_command_line():
    from pathtracerpython_amd import _abi
    from pathtracerpython_amd import main as cli
    assert _abi.PT_FLAG_LENS == 1 << 9 and _abi.PT_API_VERSION == 7
    assert C.sizeof(_abi.PtLens) == 16
    hdr = open(os.path.join(ROOT, "include", "pt_capi.h")).read()
    assert "#define PT_FLAG_LENS (1u << 9)" in hdr and "pt_scene_create_lens" in hdr
    a = cli.setup(["s.sdl", "--aperture", "0.25", "--focus-z", "-24", "--aa"])
    cli.check_args(a)
    assert cli.lens_arg(a) == (0.25, -24.0) and cli.lens_arg(cli.setup(["s.sdl"])) is None
    for argv in (["s.sdl", "--aperture", "0.25"], ["s.sdl", "--focus-z", "-24"]):
        with pytest.raises(SystemExit, match="go together"):
            cli.check_args(cli.setup(argv))
    with pytest.raises(SystemExit, match="--devices 1"):
        cli.check_args(cli.setup(["s.sdl", "--aperture", "0.25", "--focus-z", "-24", "--devices", "2"]))
    for extra in (["--noise", "0.05", "-r", "16"], ["--chunk-spp", "2", "--checkpoint", "f.npz"],
                  ["--local-devices", "1"], ["--denoise", "-r", "4"]):
        cli.check_args(cli.setup(["s.sdl", "--aperture", "0.25", "--focus-z", "-24"] + extra))
