"""Antialiasing on the host (PT_FLAG_AA, include/pt_capi.h; pt_path.h aa_jitter,
aa_dir, AaRay with either sink): the rule's helpers against their numpy
restatement bit for bit, the sample loop compiled for the host against the
oracle on shifted screen windows (tests/aa_ref.py), the stop rule on
antialiased frames, and the checkpoint keys.  The GPU cases are
tests/test_gpu_aa.py."""
import ctypes as C
import os

import numpy as np
import pytest

import hostlib
import aa_ref
from adaptive_sim import histogram, simulate
from conftest import ROOT, quad_scene

from pathtracerpython_amd import adaptive, progressive
from pathtracerpython_amd._abi import PT_FLAG_AA, PT_FLAG_RR, make_params
from pathtracerpython_amd.pack import pack_scene

_dp = C.POINTER(C.c_double)
_up = C.POINTER(C.c_uint32)


@pytest.fixture(scope="module")
def aa_host(tmp_path_factory):
    """tests/hostcheck/pt_aa_host.cpp built by the hostcheck Makefile into a
    temporary directory."""
    lib = hostlib.build(tmp_path_factory.mktemp("aa_host"), "pt_aa_host")
    lib.hc_aa_jitter.restype = None
    lib.hc_aa_jitter.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, _dp]
    lib.hc_aa_dir.restype = C.c_int
    lib.hc_aa_dir.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_double,
                              C.c_double, _dp, _dp]
    lib.hc_render_aa.restype = C.c_int
    lib.hc_accum_aa.restype = C.c_int
    lib.hc_accum_aa.argtypes = [C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_uint32,
                                C.c_uint32, C.c_uint32, _dp, _dp, _up]
    return lib


def host_aa(lib, pk, p, lanes=1, force64=False):
    """(sum, S, Q) [H, W, 3] of the host's antialiased sample loop."""
    H, W = p.height, p.width
    a, S, Q = np.zeros((H, W, 3)), np.zeros((H, W, 3)), np.zeros((H, W, 3))
    rc = lib.hc_render_aa(C.byref(pk.desc), C.byref(p), int(force64), int(lanes),
                          a.ctypes.data_as(_dp), S.ctypes.data_as(_dp), Q.ctypes.data_as(_dp))
    assert rc == 0
    return a, S, Q


@pytest.fixture(scope="module")
def ref12(cornell):
    """Cornell 12x12, 8 samples, 3 bounces, seed 9: the per-sample colours of
    the rule, with every branch of the restart loop covered."""
    c = aa_ref.aa_samples(cornell, 12, 12, 3, 9, 8)
    me, ml, ae = aa_ref.coverage(c, pack_scene(cornell).light_rgb)
    print(f"coverage 12x12: mixed-escape {me}, mixed-light {ml}, all-escape {ae}")
    assert me >= 1 and ml >= 1 and ae >= 1
    return c


@pytest.fixture(scope="module")
def ref16(cornell):
    """Cornell 16x16, 17 samples, 3 bounces, seed 9 (the adaptive cases)."""
    return aa_ref.to_image(aa_ref.aa_samples(cornell, 16, 16, 3, 9, 17), 16, 16)


# ------------------------------------------------------------ the helpers --
@pytest.mark.parametrize("W,H", [(7, 5), (1, 1), (3, 1)])
def test_jitter_and_direction_are_numpy_bit_for_bit(aa_host, cornell, W, H):
    pk = pack_scene(cornell)
    for ix in range(W):
        for iy in range(H):
            k = ix * H + iy
            for s in (0, 1, 5, 1000003):
                j = np.zeros(2)
                aa_host.hc_aa_jitter(9, k, s, j.ctypes.data_as(_dp))
                jx, jy = aa_ref.jitter(9, k, s)
                assert j[0] == jx and j[1] == jy
                assert -0.5 <= jx < 0.5 and -0.5 <= jy < 0.5
                win, d0 = np.zeros(4), np.zeros(3)
                rc = aa_host.hc_aa_dir(C.addressof(pk.desc), W, H, ix, iy, float(jx), float(jy),
                                       win.ctypes.data_as(_dp), d0.ctypes.data_as(_dp))
                assert rc == 0
                want_d, want_w = aa_ref.direction(pk.ortho, pk.eye, W, H, ix, iy, jx, jy)
                assert np.array_equal(win.view(np.uint64), want_w.view(np.uint64))
                assert np.array_equal(d0.view(np.uint64), want_d.view(np.uint64))
                if W == 1:   # dx = 0: the window's x bounds do not move
                    assert win[0] == pk.ortho[0] and win[2] == pk.ortho[2]
                if H == 1:
                    assert win[1] == pk.ortho[1] and win[3] == pk.ortho[3]


def test_jitter_is_keyed_by_seed_pixel_and_sample():
    a = aa_ref.jitter(9, 3, 4)
    assert a == aa_ref.jitter(9, 3, 4)
    assert a != aa_ref.jitter(10, 3, 4) and a != aa_ref.jitter(9, 4, 4) and a != aa_ref.jitter(9, 3, 5)
    assert a != aa_ref.jitter(9 + (1 << 32), 3, 4)   # the key's high word counts


# --------------------------------------------------------- the sample loop --
@pytest.mark.parametrize("lanes", [1, 4, 8])
def test_host_sample_loop_matches_the_oracle(aa_host, cornell, ref12, lanes):
    pk = pack_scene(cornell)
    a, S, Q = host_aa(aa_host, pk, make_params(12, 12, 8, 3, 9, PT_FLAG_AA), lanes)
    want = aa_ref.to_image(ref12, 12, 12)
    da = float(np.abs(a - want.sum(axis=0)).max())
    dS = float(np.abs(S - want.sum(axis=0)).max())
    dQ = float(np.abs(Q - (want ** 2).sum(axis=0)).max())
    print(f"lanes {lanes}: |sum| {da:.3e} |S| {dS:.3e} |Q| {dQ:.3e}")
    assert da <= 1e-12 and dS <= 1e-12 and dQ <= 1e-12


def test_host_sample_loop_uneven_lanes(aa_host, cornell):
    """7x5, 5 samples on 4 lanes: lanes of 2 and 1 samples; W != H."""
    pk = pack_scene(cornell)
    want = aa_ref.to_image(aa_ref.aa_samples(cornell, 7, 5, 3, 9, 5), 7, 5)
    a, S, Q = host_aa(aa_host, pk, make_params(7, 5, 5, 3, 9, PT_FLAG_AA), 4)
    assert np.abs(a - want.sum(axis=0)).max() <= 1e-12
    assert np.abs(S - want.sum(axis=0)).max() <= 1e-12
    assert np.abs(Q - (want ** 2).sum(axis=0)).max() <= 1e-12


def test_host_sample_ranges_and_rr(aa_host, cornell, ref12):
    pk = pack_scene(cornell)
    want = aa_ref.to_image(ref12, 12, 12)
    a, _, _ = host_aa(aa_host, pk, make_params(12, 12, 3, 3, 9, PT_FLAG_AA, sample_begin=5))
    assert np.abs(a - want[5:8].sum(axis=0)).max() <= 1e-12
    a, S, _ = host_aa(aa_host, pk, make_params(12, 12, 8, 0, 9, PT_FLAG_AA))
    assert not a.any() and not S.any()
    c = aa_ref.to_image(aa_ref.aa_samples(cornell, 8, 8, 4, 9, 4, flags=PT_FLAG_RR, rr_depth=1), 8, 8)
    a, _, _ = host_aa(aa_host, pk, make_params(8, 8, 4, 4, 9, PT_FLAG_AA | PT_FLAG_RR, 1))
    assert np.abs(a - c.sum(axis=0)).max() <= 1e-12


def test_hybrid_equals_forced_f64(aa_host, cornell, tmp_path):
    """Jittered directions are new ground for the eye-frame filter records."""
    for sc, p in ((cornell, make_params(32, 32, 4, 4, 9, PT_FLAG_AA)),
                  (quad_scene(tmp_path, 3), make_params(12, 12, 3, 4, 3, PT_FLAG_AA))):
        pk = pack_scene(sc)
        a, S, Q = host_aa(aa_host, pk, p)
        b, S64, Q64 = host_aa(aa_host, pk, p, force64=True)
        assert np.array_equal(a, b) and np.array_equal(S, S64) and np.array_equal(Q, Q64)
        assert a.any()


def test_bvh_scene_matches_the_oracle(aa_host, mesh_golden):
    sc, _ = mesh_golden
    want = aa_ref.to_image(aa_ref.aa_samples(sc, 12, 12, 3, 5, 2), 12, 12)
    a, S, _ = host_aa(aa_host, pack_scene(sc), make_params(12, 12, 2, 3, 5, PT_FLAG_AA))
    assert np.abs(a - want.sum(axis=0)).max() <= 1e-12
    assert np.abs(S - want.sum(axis=0)).max() <= 1e-12


# --------------------------------------------------------- the adaptive rule --
# tol 0.05 with the floor 1e-3: the closest stop decision of either rule is
# 1.6e-3 relative from tol
FLOOR = 1e-3


@pytest.mark.parametrize("rule,hist", [((4, 16, 4), {4: 46, 8: 31, 12: 13, 16: 166}),
                                       ((3, 17, 5), {3: 53, 8: 31, 13: 13, 17: 159})])
def test_adaptive_rule_on_antialiased_frames(aa_host, cornell, ref16, rule, hist):
    mn, mx, st = rule
    sim = simulate(ref16[:mx], 0.05, FLOOR, mn, mx, st)
    print(f"rule {rule}: margin {sim['margin']:.3e}, counts {histogram(sim['n'])}")
    assert sim["margin"] >= 1e-6   # sums that differ by 1e-12 cannot flip a count
    assert histogram(sim["n"]) == hist
    pk = pack_scene(cornell)
    S, Q = np.zeros((16, 16, 3)), np.zeros((16, 16, 3))
    n = np.zeros((16, 16), dtype=np.uint32)
    p = make_params(16, 16, mx, 3, 9, PT_FLAG_AA)
    rc = aa_host.hc_accum_aa(C.addressof(pk.desc), C.addressof(p), 0.05, FLOOR, mn, mx, st,
                             S.ctypes.data_as(_dp), Q.ctypes.data_as(_dp), n.ctypes.data_as(_up))
    assert rc == len(sim["passes"])
    assert np.array_equal(n, sim["n"])
    assert np.abs(S - sim["S"]).max() <= 1e-12 and np.abs(Q - sim["Q"]).max() <= 1e-12


# ------------------------------------------------------------- checkpoints --
def test_checkpoint_keys(packed, tmp_path):
    old = {"scene": progressive.scene_fingerprint(packed), "width": 8, "height": 8, "spp": 4,
           "bounces": 2, "seed": 9, "rr": False, "rr_depth": 3, "chunk_spp": 2}
    off = progressive.run_key(packed, 8, 8, 4, 2, 9, False, 3, 2)
    on = progressive.run_key(packed, 8, 8, 4, 2, 9, False, 3, 2, aa=True)
    assert off == old and "aa" not in off          # an old key dict compares equal
    assert on == {**old, "aa": True}
    ck = progressive.Checkpoint(tmp_path / "p.npz")
    ck.save(on, np.zeros((8, 8, 3)), 2)
    assert ck.load(on)[1] == 2
    with pytest.raises(ValueError, match="another render"):
        ck.load(off)                                # an AA file without --aa
    ck.save(off, np.zeros((8, 8, 3)), 2)
    with pytest.raises(ValueError, match="another render"):
        ck.load(on)                                 # a non-AA file with --aa

    olda = {"scene": progressive.scene_fingerprint(packed), "width": 8, "height": 8,
            "bounces": 2, "seed": 9, "rr": False, "rr_depth": 3, "lanes_per_pixel": 4}
    offa = adaptive.accum_key(packed, 8, 8, 2, 9, False, 3, 4)
    ona = adaptive.accum_key(packed, 8, 8, 2, 9, False, 3, 4, aa=True)
    assert offa == olda and ona == {**olda, "aa": True}
    ca = adaptive.AccumCheckpoint(tmp_path / "a.npz")
    z = (np.zeros((8, 8, 3)), np.zeros((8, 8, 3)), np.zeros((8, 8), dtype=np.uint32))
    ca.save(ona, {"tol": 0.05}, *z, [(64, 256)])
    assert ca.load(ona)["passes"] == [(64, 256)]
    with pytest.raises(ValueError, match="another render"):
        ca.load(offa)
    ca.save(offa, {"tol": 0.05}, *z, [])
    with pytest.raises(ValueError, match="another render"):
        ca.load(ona)


def test_flag_travels(monkeypatch):
    """--aa reaches the parameters; the ABI names the bit."""
    from pathtracerpython_amd import _abi
    from pathtracerpython_amd import main as cli
    assert _abi.PT_FLAG_AA == 1 << 8 and _abi.PT_API_VERSION == 7
    assert cli.setup(["s.sdl", "--aa"]).aa and not cli.setup(["s.sdl"]).aa
    a = cli.setup(["s.sdl", "--aa", "--noise", "0.05", "-r", "16"])
    assert cli.adaptive_args(a)["aa"] is True
    hdr = open(os.path.join(ROOT, "include", "pt_capi.h")).read()
    assert "#define PT_FLAG_AA (1u << 8)" in hdr
