"""The ray form of the wavefront state machine on the host (pt_wavefront.h
WfRays, wf_rays_primary_step, wf_finish's ray mode, wf_begin_bounce_rays:
a primary query per record, its hit cached, the record in the place of the
pixel; tests/hostcheck/pt_rays_wf_host.cpp) against the single kernel's lane
code (pt_rays_host.cpp hc_radiance: render_lane_cached over RayHit, both
sinks) bit for bit and against the oracle's per-sample
colours (tests/rays_ref.py).  The GPU cases are
tests/test_gpu_rays_wavefront.py."""
import ctypes as C
import os

import numpy as np
import pytest

import hostlib
import deep_scenes
import rays_ref
from conftest import ROOT

from pathtracerpython_amd import _abi
from pathtracerpython_amd._abi import PT_FLAG_AA, PT_FLAG_RR, make_params, make_rays
from pathtracerpython_amd.pack import pack_scene

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)
_lp = C.POINTER(C.c_int64)
TOL = 1e-12   # the project's f64 bar

# (n_rays, spp, bounces, rr_depth or None, sample_begin): every n_rays, spp and
# bounce count of the issue, Russian roulette from depth 1 and sample_begin 5
MATRIX = ((1, 1, 3, None, 0), (63, 5, 3, None, 0), (64, 8, 3, None, 0), (65, 8, 1, None, 0), (257, 1, 3, None, 0),
          (64, 5, 0, None, 0), (65, 8, 3, 1, 0), (63, 8, 3, None, 5))
# the oracle's cases: rays_ref.PARITY_CASES' BVH scenes, and a short batch each
# with Russian roulette from depth 1 and from sample 5
ORACLE = tuple(c for c in rays_ref.PARITY_CASES if c[0] in ("mesh", "multi")) + (
    ("mesh", 16, 5, 3, 1, 0), ("mesh", 16, 5, 3, None, 5))


@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    """pt_rays_wf_host.cpp (the state machine, on the buffers of the
    antialiased and the lens one) and pt_rays_host.cpp (the lane code)."""
    tmp = tmp_path_factory.mktemp("rays_wf_host")
    wf, lane = hostlib.build(tmp, "pt_rays_wf_host"), hostlib.build(tmp, "pt_rays_host")
    wf.hc_rays_wf.restype = C.c_int
    wf.hc_rays_wf.argtypes = [C.c_void_p, _dp, C.c_void_p, C.c_int64, C.c_void_p, C.c_uint32, C.c_int, _dp, _dp,
                              _dp, _ip, _ip, _lp]
    wf.hc_aa_wf_render.restype = C.c_int
    wf.hc_aa_wf_render.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, _dp, _ip, _ip, C.c_int32]
    wf.hc_flag_rays_single.restype = C.c_uint32
    lane.hc_radiance.restype = C.c_int
    lane.hc_radiance.argtypes = [C.c_void_p, _dp, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_int32,
                                 _dp, _dp, _dp, _ip]
    return wf, lane


@pytest.fixture(scope="module")
def benches(tmp_path_factory, cornell, mesh_golden):
    """name -> rays_ref.Bench, made at first use; the batch's coverage is
    asserted before anything is compared on it."""
    made = {}

    def get(name):
        if name not in made:
            b = rays_ref.Bench(rays_ref.make_scene(name, tmp_path_factory.mktemp(name), cornell, mesh_golden))
            esc, light, spec = rays_ref.first_hits(b.pk, b.o, b.d)
            print(f"{name}: batch of {len(b.o)}: {esc} escapes, {light} light hits, {spec} specular first hits")
            assert esc >= 1 and light >= 1 and spec >= 1
            assert b.outside[:64].any() and not b.outside[:64].all()
            made[name] = b
        return made[name]
    return get


def box_ptr(box):
    return None if box is None else np.ascontiguousarray(box, dtype=np.float64).ctypes.data_as(_dp)


def params(spp, bounces, rr_depth=None, sample_begin=0, seed=9):
    return make_params(1, 1, spp, bounces, seed, 0 if rr_depth is None else PT_FLAG_RR,
                       3 if rr_depth is None else rr_depth, sample_begin=sample_begin)


def wf_radiance(lib, pk, box, o, d, keys, p, split, fresh=1):
    """(sum, S, Q, queried [n], steps [2], peak [2]) of the state machine."""
    rec = make_rays(o, d, keys)
    n = rec.shape[0]
    a, S, Q = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, 3))
    queried = np.full(n, -1, dtype=np.int32)
    steps = np.zeros(2, dtype=np.int32)
    peak = np.zeros(2, dtype=np.int64)
    rc = lib.hc_rays_wf(C.addressof(pk.desc), box_ptr(box), C.c_void_p(rec.ctypes.data), n, C.addressof(p),
                        int(split), int(fresh), a.ctypes.data_as(_dp), S.ctypes.data_as(_dp), Q.ctypes.data_as(_dp),
                        queried.ctypes.data_as(_ip), steps.ctypes.data_as(_ip), peak.ctypes.data_as(_lp))
    assert rc == 0
    return a, S, Q, queried, steps, peak


def lane_code(lib, pk, box, o, d, keys, p, lanes, force64=False):
    """(sum, S, Q, route) of the single kernel's lane code."""
    rec = make_rays(o, d, keys)
    n = rec.shape[0]
    a, S, Q = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, 3))
    route = np.zeros(n, dtype=np.int32)
    rc = lib.hc_radiance(C.addressof(pk.desc), box_ptr(box), C.c_void_p(rec.ctypes.data), n, C.addressof(p),
                         int(force64), int(lanes), a.ctypes.data_as(_dp), S.ctypes.data_as(_dp),
                         Q.ctypes.data_as(_dp), route.ctypes.data_as(_ip))
    assert rc == 0
    return a, S, Q, route


def same(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def mid(c):
    return "n%d-spp%d-b%d%s%s" % (c[0], c[1], c[2], "" if c[3] is None else "-rr%d" % c[3],
                                  "-s%d" % c[4] if c[4] else "")


# --------------------------------------------------------- the lane code --
@pytest.mark.parametrize("boxed", [True, False], ids=["box", "plain"])
@pytest.mark.parametrize("name", ["mesh", "multi"])
@pytest.mark.parametrize("case", MATRIX, ids=mid)
def test_state_machine_is_the_lane_code_bit_for_bit(libs, benches, case, name, boxed):
    """Mean (the sum before its division), S and Q; 1 and 4 slots per record;
    the route per record; the shade steps that found work."""
    wf, lane = libs
    n, spp, bounces, rr_depth, s0 = case
    b = benches(name)
    box = b.box if boxed else None
    p = params(spp, bounces, rr_depth, s0)
    for split in (1, 4):
        if split > spp:
            continue
        a, S, Q, route = lane_code(lane, b.pk, box, b.o[:n], b.d[:n], b.keys[:n], p, split)
        ga, gS, gQ, queried, steps, _ = wf_radiance(wf, b.pk, box, b.o[:n], b.d[:n], b.keys[:n], p, split)
        assert same(ga, a) and same(gS, S) and same(gQ, Q)
        per_slot = -(-spp // split)
        assert steps.max() <= per_slot * bounces + 2
        if bounces == 0:
            assert not ga.any() and not gS.any() and not gQ.any() and list(steps) == [1, 1]
            assert (queried == 0).all()
        else:
            assert n < 8 or a.any()
            # a closest query for the records inside the frame and for no other
            assert np.array_equal(queried, 1 - route)
            if boxed:
                assert np.array_equal(queried, (~b.outside[:n]).astype(np.int32))


@pytest.mark.parametrize("name", ["mesh", "multi"])
def test_out_of_frame_records_take_the_f64_primary(libs, benches, name):
    """Records outside the frame and one NaN origin issue no closest query and
    equal the forced-f64 lane code bit for bit; the others issue one."""
    wf, lane = libs
    b = benches(name)
    n = 64
    o = b.o[:n].copy()
    ins = np.flatnonzero(~b.outside[:n])
    o[ins[3], 1] = np.nan
    outside = b.outside[:n].copy()
    outside[ins[3]] = True
    p = params(5, 3)
    with np.errstate(invalid="ignore"):
        for box in (b.box, None):
            for split in (1, 4):
                ga, gS, gQ, queried, _, _ = wf_radiance(wf, b.pk, box, o, b.d[:n], b.keys[:n], p, split)
                f64 = lane_code(lane, b.pk, box, o, b.d[:n], b.keys[:n], p, split, force64=True)
                hyb = lane_code(lane, b.pk, box, o, b.d[:n], b.keys[:n], p, split)
                if box is not None:
                    assert np.array_equal(queried, (~outside).astype(np.int32))
                assert not queried[outside].any() and queried.any()
                assert np.array_equal(queried, 1 - hyb[3])
                for got, want, h in zip((ga, gS, gQ), f64[:3], hyb[:3]):
                    assert same(got[queried == 0], want[queried == 0])
                    assert same(got, h)


# ------------------------------------------------------------ the oracle --
@pytest.mark.parametrize("boxed", [True, False], ids=["box", "plain"])
@pytest.mark.parametrize("case", ORACLE, ids=rays_ref.case_id)
def test_oracle_parity(libs, benches, case, boxed):
    """Every record's mean, S and Q within 1e-12 of the oracle's per-sample
    colours, none excluded; 1 and 4 slots per record."""
    wf, _ = libs
    name, n, spp, bounces, rr_depth, s0 = case
    b = benches(name)
    want = b.samples(n, bounces, rr_depth, s0, spp)
    p = params(spp, bounces, rr_depth, s0)
    for split in (1, 4):
        if split > spp:
            continue
        a, S, Q, _, _, _ = wf_radiance(wf, b.pk, b.box if boxed else None, b.o[:n], b.d[:n], b.keys[:n], p, split)
        for what, got, ref in (("mean", a / spp, want.sum(axis=0) / spp), ("S", S, want.sum(axis=0)),
                               ("Q", Q, (want ** 2).sum(axis=0))):
            err = np.abs(got - ref)
            print(f"{rays_ref.case_id(case)} slots {split}: |{what}| {err.max():.3e}")
            assert err.max() <= TOL, f"{what} off by {err.max():.3e} at record {int(err.max(axis=1).argmax())}"


# ----------------------------------------------------------- the buffers --
def test_stale_buffers(libs, benches):
    """fresh = 0: the buffers hold another run's state — a wider ray launch
    with another seed and Russian roulette, an antialiased frame of the same
    scene — or the 0x55 fill (fresh = 1): step 0 and the primary step
    initialise everything a run reads, the primary queries' marker included
    (the in-frame and the f64 records swap places between the two batches)."""
    wf, _ = libs
    b = benches("mesh")
    n = 65
    p = params(5, 3)
    clean = wf_radiance(wf, b.pk, b.box, b.o[:n], b.d[:n], b.keys[:n], p, 2)[:3]
    other = make_params(1, 1, 8, 2, 11, PT_FLAG_RR, 0)
    wf_radiance(wf, b.pk, b.box, b.o[1:n + 40], b.d[1:n + 40], b.keys[1:n + 40], other, 8)
    got = wf_radiance(wf, b.pk, b.box, b.o[:n], b.d[:n], b.keys[:n], p, 2, fresh=0)[:3]
    assert all(same(x, y) for x, y in zip(got, clean))
    out = np.zeros((12, 12, 3))
    steps = C.c_int32(0)
    busy = np.zeros(64, dtype=np.int32)
    q = make_params(12, 12, 8, 3, 11, PT_FLAG_AA)
    assert wf.hc_aa_wf_render(C.addressof(b.pk.desc), C.addressof(q), 4, 0, out.ctypes.data_as(_dp),
                              C.byref(steps), busy.ctypes.data_as(_ip), 64) == 0
    got = wf_radiance(wf, b.pk, b.box, b.o[:n], b.d[:n], b.keys[:n], p, 2, fresh=0)[:3]
    assert all(same(x, y) for x, y in zip(got, clean))


# ----------------------------------------------------------- deep stacks --
def ray_batch(pk, n):
    o, _, d, keys = rays_ref.batch(pk, n)
    inb = ~np.all(o == np.array(rays_ref.OFF_AXIS[1]), axis=1)
    return o, d, keys, np.concatenate([o[inb].min(axis=0), o[inb].max(axis=0)])


def test_comb_on_the_bound_goes_through_and_one_past_it_is_refused(libs, tmp_path):
    wf, lane = libs
    (tmp_path / "b").mkdir()
    pk = pack_scene(deep_scenes.comb_scene(tmp_path / "b", *deep_scenes.COMB_BELOW))   # qstack 48
    o, d, keys, box = ray_batch(pk, 65)
    p = params(5, 3, 1)
    for split in (1, 4):
        a, S, Q, _ = lane_code(lane, pk, box, o, d, keys, p, split)
        ga, gS, gQ, queried, _, _ = wf_radiance(wf, pk, box, o, d, keys, p, split)
        assert a.any() and same(ga, a) and same(gS, S) and same(gQ, Q) and queried.any() and not queried.all()
    (tmp_path / "a").mkdir()
    above = pack_scene(deep_scenes.comb_scene(tmp_path / "a", *deep_scenes.COMB_ABOVE))   # qstack 49
    rec = make_rays(o, d, keys)
    z = np.zeros((65, 3))
    rc = wf.hc_rays_wf(C.addressof(above.desc), box_ptr(box), C.c_void_p(rec.ctypes.data), 65, C.addressof(p), 1, 1,
                       z.ctypes.data_as(_dp), z.ctypes.data_as(_dp), z.ctypes.data_as(_dp), None, None, None)
    assert rc == -3   # (the host entries' code for a scene the wavefront kernels do not take)


def test_sliver_scene_fills_the_stacks_from_ray_origins(libs, tmp_path):
    """The primary walks from the batch's origins hold more entries than the
    walk kernels' shared-memory part (16), and the result is the lane code's."""
    wf, lane = libs
    pk = pack_scene(deep_scenes.sliver_scene(tmp_path))
    o, d, keys, box = ray_batch(pk, 64)
    p = params(2, 2)
    a, S, Q, _ = lane_code(lane, pk, box, o, d, keys, p, 2)
    ga, gS, gQ, queried, _, peak = wf_radiance(wf, pk, box, o, d, keys, p, 2)
    print(f"sliver: primary walks' peak stack {peak[0]}, node visits above 16 entries {peak[1]}")
    assert deep_scenes.WALK_STACK_LDS < peak[0] <= deep_scenes.WALK_STACK and peak[1] > 0
    assert same(ga, a) and same(gS, S) and same(gQ, Q) and queried.any()


# ----------------------------------------------------------------- the ABI --
def test_abi(libs):
    wf, _ = libs
    assert wf.hc_ray_size() == 56 and wf.hc_launch_info_size() == 16 and C.sizeof(_abi.PtLaunchInfo) == 16
    assert _abi.PT_API_VERSION == 7 and wf.hc_api_version() == 7
    assert _abi.PT_FLAG_RAYS_SINGLE == 1 << 10 == wf.hc_flag_rays_single()
    hdr = open(os.path.join(ROOT, "include", "pt_capi.h")).read()
    assert "#define PT_FLAG_RAYS_SINGLE (1u << 10)" in hdr and "#define PT_API_VERSION 7" in hdr
