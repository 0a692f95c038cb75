"""Rays of any direction and origin on the host: the reference for them
(oracle.radiance, pt_oracle.c oracle_radiance) pinned three ways — against
rays_ref.ray_samples on the rays that cross the screen plane, against the
Python restatement of tests/rays_any_ref.py, against goldens of the unmodified
reference (tests/golden/rays_*.npz, gen_golden.py rays) — and then the host
twins on the classes of tests/rays_any_ref.py: the lane code
(tests/hostcheck/pt_rays_host.cpp), the wavefront state machine
(pt_rays_wf_host.cpp) and the list pass (pt_rays_list_host.cpp).  The GPU
cases are tests/test_gpu_rays_any.py."""
import ctypes as C
import os

import numpy as np
import pytest

import hostlib
import adaptive_sim
import rays_adaptive_ref as adaptive_ref
import rays_any_ref as ra
import rays_ref
from conftest import GOLDEN, random_scene
from oracle import oracle

from pathtracerpython_amd._abi import PT_FLAG_RR, make_adapt, make_params, make_rays

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)
_lp = C.POINTER(C.c_int64)
_up = C.POINTER(C.c_uint32)
SCENES = ("cornell", "mesh", "rand")
ALL = ra.CLASS_NAMES + ("overflow",)


@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    """(lane code, wavefront state machine, list pass, walk check) built as
    their own tests build them."""
    tmp = tmp_path_factory.mktemp("rays_any_host")
    lane, wf = hostlib.build(tmp, "pt_rays_host"), hostlib.build(tmp, "pt_rays_wf_host")
    lane.hc_radiance.restype = C.c_int
    lane.hc_radiance.argtypes = [C.c_void_p, _dp, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_int32,
                                 _dp, _dp, _dp, _ip]
    wf.hc_rays_wf.restype = C.c_int
    wf.hc_rays_wf.argtypes = [C.c_void_p, _dp, C.c_void_p, C.c_int64, C.c_void_p, C.c_uint32, C.c_int, _dp, _dp,
                              _dp, _ip, _ip, _lp]
    lst = hostlib.build(tmp, "pt_rays_list_host")
    lst.hc_rays_list_pass.restype = C.c_int
    lst.hc_rays_list_pass.argtypes = [C.c_void_p, _dp, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_int,
                                      C.c_uint32, _up, C.c_uint32, _dp, _dp, _up]
    walk = hostlib.build(tmp, "pt_walk_lines_host")
    walk.hc_walk_lines.restype = C.c_int
    walk.hc_walk_lines.argtypes = [C.c_void_p, _dp, _dp, C.c_int64, _lp]
    return lane, wf, lst, walk


@pytest.fixture(scope="module")
def rays(tmp_path_factory, cornell, mesh_golden):
    """name -> rays_any_ref.Rays; the coverage is asserted when it is made."""
    def get(name):
        make = {"cornell": lambda: cornell, "mesh": lambda: mesh_golden[0],
                "rand": lambda: random_scene(tmp_path_factory.mktemp("rand"), 300, 21)}[name]
        fresh = name not in ra._made
        R = ra.rays_of(name, make)
        if fresh:
            R.check_coverage()
        return R
    return get


def box_ptr(box):
    return None if box is None else np.ascontiguousarray(box, dtype=np.float64).ctypes.data_as(_dp)


def params(spp, rr_depth=None, sample_begin=0):
    return make_params(1, 1, spp, ra.BOUNCES, ra.SEED, 0 if rr_depth is None else PT_FLAG_RR,
                       3 if rr_depth is None else rr_depth, sample_begin=sample_begin)


def lane_code(lib, pk, box, o, d, keys, p, lanes=1, force64=False):
    """(sum, S, Q, route) of hc_radiance."""
    rec = make_rays(o, d, keys)
    n = rec.shape[0]
    a, S, Q = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, 3))
    route = np.zeros(n, dtype=np.int32)
    rc = lib.hc_radiance(C.addressof(pk.desc), box_ptr(box), C.c_void_p(rec.ctypes.data), n, C.addressof(p),
                         int(force64), int(lanes), a.ctypes.data_as(_dp), S.ctypes.data_as(_dp),
                         Q.ctypes.data_as(_dp), route.ctypes.data_as(_ip))
    assert rc == 0
    return a, S, Q, route


def wf_code(lib, pk, box, o, d, keys, p, split):
    """(sum, S, Q, queried) of hc_rays_wf."""
    rec = make_rays(o, d, keys)
    n = rec.shape[0]
    a, S, Q = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, 3))
    queried = np.full(n, -1, dtype=np.int32)
    steps, peak = np.zeros(2, dtype=np.int32), np.zeros(2, dtype=np.int64)
    rc = lib.hc_rays_wf(C.addressof(pk.desc), box_ptr(box), C.c_void_p(rec.ctypes.data), n, C.addressof(p),
                        int(split), 1, a.ctypes.data_as(_dp), S.ctypes.data_as(_dp), Q.ctypes.data_as(_dp),
                        queried.ctypes.data_as(_ip), steps.ctypes.data_as(_ip), peak.ctypes.data_as(_lp))
    assert rc == 0
    return a, S, Q, queried


def same(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def moments(want):
    return want.sum(axis=0) / len(want), want.sum(axis=0), (want ** 2).sum(axis=0)


# ------------------------------------------------- the reference, pinned --
@pytest.mark.parametrize("rr_depth", [None, 1], ids=["plain", "rr1"])
@pytest.mark.parametrize("name", ["cornell", "mesh"])
def test_oracle_entry_is_ray_samples_bit_for_bit(cornell, mesh_golden, name, rr_depth):
    """On rays_ref.batch(pk, 257), whose rays the descriptor with eye = o
    reaches, the new entry is the old reference bit for bit: path_sample is
    its ray set-up in front of the same body."""
    scene = cornell if name == "cornell" else mesh_golden[0]
    b = rays_ref.Bench(scene)
    flags = 0 if rr_depth is None else PT_FLAG_RR
    want = rays_ref.ray_samples(scene, b.o, b.p, b.keys, 3, 9, 3, sample_begin=2, flags=flags, rr_depth=rr_depth or 3)
    got = oracle.radiance(b.pk, b.o, b.d, b.keys, 3, 9, 3, 2, flags, rr_depth or 3)
    assert want.any() and same(got, want)


def test_diffuse_dir_is_the_reference_formula():
    """oracle.diffuse_dir (main.py:242-247), the one primitive the restatement
    takes that no golden KAT holds on its own: numpy's formula within 4 ulp of
    a unit vector's components, over the draws' range."""
    rng = np.random.default_rng(2)
    u = np.concatenate([rng.uniform(0, 1, size=(500, 2)), [[0.0, 0.0], [1.0 - 2.0 ** -24, 1.0 - 2.0 ** -24]]])
    for a, b in u:
        phi, theta = np.arccos(np.sqrt(a)), 6.28 * b
        v = np.array([np.sin(phi) * np.cos(theta), np.sin(phi) * np.sin(theta), np.cos(phi)])
        v = v / np.linalg.norm(v)
        assert np.abs(oracle.diffuse_dir(a, b) - v).max() <= 4 * 2.0 ** -52


@pytest.mark.parametrize("name", SCENES)
def test_oracle_entry_is_the_restatement_bit_for_bit(rays, name):
    """All 257 records at 5 samples; every third with Russian roulette from
    depth 1 and from sample 5; the overflow class."""
    R = rays(name)
    got, _ = R.restated()
    assert same(got, R.samples("cat", ns=ra.SPEC_SAMPLES)) and not np.isnan(got).any()
    sel = slice(0, None, 3)
    o, d, k = R.o[sel], R.d[sel], R.keys[sel]
    rr, _ = ra.restate(R.pk, o, d, k, ra.BOUNCES, ra.SEED, 3, sample_begin=5, rr_depth=1)
    assert same(rr, oracle.radiance(R.pk, o, d, k, ra.BOUNCES, ra.SEED, 3, 5, PT_FLAG_RR, 1))
    assert not same(rr, oracle.radiance(R.pk, o, d, k, ra.BOUNCES, ra.SEED, 3, 5))   # (the roulette acts)
    o, d, k = R.overflow
    assert same(ra.restate(R.pk, o, d, k, ra.BOUNCES, ra.SEED, 2)[0], R.samples("overflow", ns=2))


@pytest.mark.parametrize("fixture,scene,camera", ra.GOLDENS, ids=[g[0] for g in ra.GOLDENS])
def test_goldens_of_the_unmodified_reference(libs, cornell, mesh_golden, fixture, scene, camera):
    """The reference's own colours of caller-chosen rays (gen_golden.py rays):
    the oracle entry and the host lane code within 1e-12; the fixture holds
    the rays rays_any_ref.golden_rays describes."""
    g = np.load(os.path.join(GOLDEN, fixture))
    assert sorted(g.files) == ["bounces", "colors", "d", "keys", "o", "seed", "spp"]
    o, d = ra.golden_rays(camera)
    assert same(g["d"], d) and same(g["o"], np.broadcast_to(o, d.shape).copy())
    assert np.array_equal(g["keys"], np.arange(len(d))) and len(d) >= 25
    spp, B, seed = int(g["spp"]), int(g["bounces"]), int(g["seed"])
    assert (spp, B, seed) == ra.GOLDEN_FRAME
    sc = cornell if scene == "cornell" else mesh_golden[0]
    from pathtracerpython_amd.pack import pack_scene
    pk = pack_scene(sc)
    want = g["colors"]
    ref = oracle.radiance(pk, g["o"], g["d"], g["keys"], B, seed, spp).sum(axis=0) / spp
    p = make_params(1, 1, spp, B, seed)
    host = lane_code(libs[0], pk, None, g["o"], g["d"], g["keys"], p)[0] / spp
    print(f"{fixture}: oracle {ra.rel(ref, want):.3e}, host lane code {ra.rel(host, want):.3e}, "
          f"{int((want == 0).all(axis=1).sum())} escapes of {len(want)}")
    assert want.any() and ra.rel(ref, want) <= ra.TOL and ra.rel(host, want) <= ra.TOL


@pytest.mark.parametrize("name", SCENES)
def test_overflow_class_is_zero_in_the_reference(rays, name):
    """Lengths of 1e300 and 1e-300: the reference's norm is inf or 0, no
    triangle is hit, the value is 0 — for every record."""
    R = rays(name)
    o, d, _ = R.overflow
    assert len(o) >= 8 and (np.abs(d).max(axis=1) > 1e290).any() and (np.abs(d).max(axis=1) < 1e-290).any()
    assert not R.samples("overflow", ns=5).any()


# ---------------------------------------------------------- the lane code --
@pytest.mark.parametrize("boxed", [True, False], ids=["box", "plain"])
@pytest.mark.parametrize("name", SCENES)
def test_lane_code_against_the_oracle_entry(libs, rays, name, boxed):
    """Every class: mean, S and Q within the class's tolerance (1e-12; 8 x the
    measured host difference where that is more) of oracle.radiance, none
    excluded, at 1 and 4 lanes; forced f64 is the hybrid result bit for bit;
    Russian roulette from depth 1 and samples from 5 on all 257 records."""
    lane = libs[0]
    R = rays(name)
    box = R.box if boxed else None
    worst = {}
    for cls in ALL:
        o, d, k = R.records(cls)
        mean, S, Q = moments(R.samples(cls, ns=5))
        for lanes in (1, 4):
            a, gS, gQ, _ = lane_code(lane, R.pk, box, o, d, k, params(5), lanes)
            e = max(ra.rel(a / 5, mean), ra.rel(gS, S), ra.rel(gQ, Q))
            worst[cls] = max(worst.get(cls, 0.0), e)
            f = lane_code(lane, R.pk, box, o, d, k, params(5), lanes, force64=True)
            assert same(a, f[0]) and same(gS, f[1]) and same(gQ, f[2]), cls
            if cls == "overflow":
                assert not a.any() and not gS.any() and not gQ.any()
    print(f"{name} {'box' if boxed else 'plain'}: host lane code against the oracle entry: " +
          ", ".join(f"{c} {worst[c]:.2e}" for c in ALL))
    for cls in ALL:
        assert worst[cls] <= ra.class_tol(cls), cls
    for rr_depth, s0 in ((1, 0), (None, 5)):
        mean, S, Q = moments(R.samples("cat", rr_depth, s0, 8))
        a, gS, gQ, _ = lane_code(lane, R.pk, box, R.o, R.d, R.keys, params(8, rr_depth, s0), 4)
        assert max(ra.rel(a / 8, mean), ra.rel(gS, S), ra.rel(gQ, Q)) <= ra.TOL


def test_the_box_decides_the_route(libs, rays):
    """With the box the ortho class's origins and the inside eye take the f32
    filter's route; origins 100 and 200 from the room take the f64 primary."""
    R = rays("cornell")
    route = lane_code(libs[0], R.pk, R.box, R.o, R.d, R.keys, params(1))[3]
    assert not route[R.spans["ortho"]].any() and not route[R.spans["inside"]].any()
    far = route[R.spans["far"]]
    assert far[np.arange(len(far)) % 3 != 0].all()   # (far_class: 30, 100, 200 in turn)


# ------------------------------------------------------ the state machine --
@pytest.mark.parametrize("boxed", [True, False], ids=["box", "plain"])
@pytest.mark.parametrize("name", ["mesh", "rand"])
def test_state_machine_is_the_lane_code_bit_for_bit(libs, rays, name, boxed):
    """hc_rays_wf on every class at 1 and 4 slots per record: mean, S and Q
    are hc_radiance's bits; a closest query for the records the lane code's
    primary sends through the f32 filter and for no other.  (The scenes with a
    BVH: the wavefront kernels take no other, and hc_rays_wf answers -3 on
    Cornell, as tests/test_rays_wavefront_host.py holds it to.)"""
    lane, wf = libs[:2]
    R = rays(name)
    box = R.box if boxed else None
    for cls in ALL:
        o, d, k = R.records(cls)
        for split in (1, 4):
            a, S, Q, route = lane_code(lane, R.pk, box, o, d, k, params(5), split)
            ga, gS, gQ, queried = wf_code(wf, R.pk, box, o, d, k, params(5), split)
            assert same(ga, a) and same(gS, S) and same(gQ, Q), cls
            assert np.array_equal(queried, 1 - route), cls


# -------------------------------------------------------------- the walks --
@pytest.mark.parametrize("name", ["mesh", "rand"])
def test_walks_on_lines_with_zero_and_subnormal_components(libs, rays, name):
    """hc_bvh_check's and hc_qbvh_check's conditions on the classes' own lines
    (theirs are random: no zero component): both walks reach the leaf of every
    triangle the f64 reference says a line meets, the sign-ordered child test
    is q_child_dist bit for bit, absent children stay out, and no slab
    parameter is inf or NaN: rcp_dir gives 1e30 for a component that is zero
    or subnormal in f32 (1e-39, 1e-42, 1e-45, 1e-200), so q_slabs' "A is never
    zero" and finite products hold for a caller's direction as for a frame's."""
    R = rays(name)
    seen = 0
    for cls in ALL:
        o, d, _ = R.records(cls)
        out = (C.c_int64 * 8)()
        assert libs[3].hc_walk_lines(C.addressof(R.pk.desc), np.ascontiguousarray(o).ctypes.data_as(_dp),
                                     np.ascontiguousarray(d).ctypes.data_as(_dp), len(o), out) == 0
        hits, missed_b, missed_q, differ, tests, absent, odd, tiny = list(out)
        print(f"{name} {cls}: {hits} hits, {tests} child tests, {tiny} lines with a zero or subnormal component; "
              f"missed {missed_b} / {missed_q}, forms differ {differ}, absent let in {absent}, not finite {odd}")
        assert (missed_b, missed_q, differ, absent, odd) == (0, 0, 0, 0, 0), cls
        if cls in ("axis", "flat"):   # (all but the three with a component of 1e-30, a normal f32)
            assert tiny == len(o) - (3 if cls == "axis" else 0) and hits > 0 and tests > 0
        seen += hits
    assert seen >= 50


# ---------------------------------------------------------- the list pass --
def pass_split(L, kmin):
    cap = 1
    while cap * 2 <= min(kmin, 64):
        cap *= 2
    return min(L, cap)


def adaptive_batch(R):
    """rays_adaptive_ref.Batch of all 257 records with oracle.radiance as the
    source of the samples."""
    def source(rr_depth, ns):
        return R.samples("cat", rr_depth, 0, ns)
    return adaptive_ref.Batch(R.scene, records=(R.o, R.d, R.keys, R.box), source=source)


@pytest.mark.parametrize("rule,L", [("r4-32-4", 4), ("r3-17-5", 1)])
@pytest.mark.parametrize("name", SCENES)
def test_list_pass_is_the_simulation(libs, rays, name, rule, L):
    """An adaptive run over all 257 records through the host list pass: before
    every pass the list is the simulation's (the stop rule on the oracle
    entry's samples summed up to the counts), after it n is the simulation's
    and S and Q are within 1e-12; no stop decision within 1e-4 of the bar."""
    lst_lib = libs[2]
    R = rays(name)
    b = adaptive_batch(R)
    tol, floor, lo, hi, step = adaptive_ref.RULES[rule]
    sim = b.simulate(rule)
    samples = b.samples()
    assert sim["margin"] >= adaptive_ref.MIN_MARGIN and len(adaptive_sim.histogram(sim["n"])) >= 3
    traj = adaptive_ref.trajectory(samples, rule)
    rec = make_rays(b.o, b.d, b.keys)
    p = make_params(b.n, 1, hi, ra.BOUNCES, ra.SEED)
    ap = make_adapt(tol, hi, lo, step, floor)
    S, Q, n = np.zeros((b.n, 3)), np.zeros((b.n, 3)), np.zeros(b.n, dtype=np.uint32)
    box = np.ascontiguousarray(b.box, dtype=np.float64)
    sim_n = np.zeros(b.n, dtype=np.int64)
    worst = 0.0
    for i in range(len(traj) + 1):
        act = adaptive_sim.active_numpy(n, adaptive_sim.err_numpy(S, Q, n, floor), tol, lo, hi)
        lst = np.nonzero(act)[0].astype(np.uint32)
        wS, wQ = adaptive_sim.moments_upto(samples, sim_n)
        want = adaptive_sim.active_numpy(sim_n, adaptive_sim.err_numpy(wS, wQ, sim_n, floor), tol, lo, hi)
        assert np.array_equal(lst, np.nonzero(want)[0]), f"the list of pass {i + 1}"
        if i == len(traj):
            assert len(lst) == 0
            break
        k = adaptive_sim.k_numpy(n[lst], lo, hi, step)
        assert (len(lst), int(k.sum())) == traj[i][:2]
        rc = lst_lib.hc_rays_list_pass(C.addressof(b.pk.desc), box.ctypes.data_as(_dp), C.c_void_p(rec.ctypes.data),
                                       b.n, C.addressof(p), C.addressof(ap), 0, pass_split(L, int(k.min())),
                                       lst.ctypes.data_as(_up), len(lst), S.ctypes.data_as(_dp),
                                       Q.ctypes.data_as(_dp), n.ctypes.data_as(_up))
        assert rc == 0
        sim_n = traj[i][2]
        assert np.array_equal(n, sim_n), f"n after pass {i + 1}"
        wS, wQ = adaptive_sim.moments_upto(samples, sim_n)
        worst = max(worst, ra.rel(S, wS), ra.rel(Q, wQ))
        assert ra.rel(S, wS) <= ra.TOL and ra.rel(Q, wQ) <= ra.TOL, f"pass {i + 1}"
    print(f"{name} {rule} L={L}: {len(traj)} passes, counts {adaptive_sim.histogram(n)}, worst |S|, |Q| {worst:.3e}")
    assert np.array_equal(n, sim["n"])
