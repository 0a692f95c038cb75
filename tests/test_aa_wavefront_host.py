"""The antialiased wavefront state machine on the host (pt_wavefront.h
wf_aa_start / wf_shade_aa: a primary query per sample in the slot's own record;
tests/hostcheck/pt_aa_wf_host.cpp), in its uniform and its list form, against
the single kernel's lane code (pt_aa_host.cpp hc_render_aa: render_lane_sampled
over AaRay, both sinks) bit for bit and against the oracle's antialiased
per-sample colours (tests/aa_ref.py).  The GPU cases are
tests/test_gpu_aa_wavefront.py."""
import ctypes as C

import numpy as np
import pytest

import hostlib
import aa_ref

from pathtracerpython_amd._abi import PT_FLAG_AA, PT_FLAG_RR, make_params
from pathtracerpython_amd.pack import pack_scene

_dp = C.POINTER(C.c_double)
_up = C.POINTER(C.c_uint32)
_ip = C.POINTER(C.c_int32)

W = H = 12
BOUNCES, SEED = 3, 5
ALL = np.arange(W * H, dtype=np.uint32)


@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    """pt_aa_wf_host.cpp (the state machine) and pt_aa_host.cpp (the single
    kernel's lane code)."""
    tmp = tmp_path_factory.mktemp("aa_wf_host")
    wf, lane = hostlib.build(tmp, "pt_aa_wf_host"), hostlib.build(tmp, "pt_aa_host")
    wf.hc_aa_wf_render.restype = C.c_int
    wf.hc_aa_wf_render.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, _dp, _ip, _ip, C.c_int32]
    wf.hc_aa_wf_pass.restype = C.c_int
    wf.hc_aa_wf_pass.argtypes = [C.c_void_p, C.c_void_p, _up, C.c_uint32, C.c_uint32, C.c_uint32,
                                 C.c_uint32, C.c_uint32, C.c_int, _dp, _dp, _up, _ip, _ip, C.c_int32]
    lane.hc_render_aa.restype = C.c_int
    lane.hc_render_aa.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int32, _dp, _dp, _dp]
    return wf, lane


@pytest.fixture(scope="module")
def pk(mesh_golden):
    return pack_scene(mesh_golden[0])


@pytest.fixture(scope="module")
def frames(mesh_golden, pk):
    """Mesh scene 12x12, 3 bounces, seed 5: the oracle's 8 antialiased
    per-sample frames [8, H, W, 3]; they, and the first two of them, run every
    branch of the restart."""
    c = aa_ref.aa_samples(mesh_golden[0], W, H, BOUNCES, SEED, 8)
    for n in (8, 2):
        cov = aa_ref.coverage(c[:n], pk.light_rgb)
        print(f"coverage of the first {n} samples: {cov}")
        assert min(cov) >= 1
    return aa_ref.to_image(c, W, H)


CAP = 64


def wf_render(lib, pk, p, split, fresh=1):
    """(sum [H, W, 3], shade steps that found work, busy slots after each step)"""
    out = np.zeros((p.height, p.width, 3))
    steps = C.c_int32(0)
    busy = np.full(CAP, -1, dtype=np.int32)
    rc = lib.hc_aa_wf_render(C.addressof(pk.desc), C.addressof(p), split, fresh, out.ctypes.data_as(_dp),
                             C.byref(steps), busy.ctypes.data_as(_ip), CAP)
    assert rc == 0
    return out, steps.value, busy


def wf_pass(lib, pk, p, lst, rule, split, S, Q, n, fresh=1):
    """One list pass on copies of S, Q, n: (S, Q, n, steps, busy)."""
    S, Q, n = S.copy(), Q.copy(), n.copy()
    lst = np.ascontiguousarray(lst, dtype=np.uint32)
    steps = C.c_int32(0)
    busy = np.full(CAP, -1, dtype=np.int32)
    rc = lib.hc_aa_wf_pass(C.addressof(pk.desc), C.addressof(p), lst.ctypes.data_as(_up), len(lst), *rule,
                           split, fresh, S.ctypes.data_as(_dp), Q.ctypes.data_as(_dp),
                           n.ctypes.data_as(_up), C.byref(steps), busy.ctypes.data_as(_ip), CAP)
    assert rc == 0
    return S, Q, n, steps.value, busy


def lane_code(lib, pk, p, lanes):
    """(sum, S, Q) of render_lane_sampled over AaRay (SumSink, MomentSink), `lanes` per pixel."""
    a, S, Q = (np.zeros((p.height, p.width, 3)) for _ in range(3))
    rc = lib.hc_render_aa(C.addressof(pk.desc), C.addressof(p), 0, int(lanes), a.ctypes.data_as(_dp),
                          S.ctypes.data_as(_dp), Q.ctypes.data_as(_dp))
    assert rc == 0
    return a, S, Q


def same(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def empty(h=H, w=W, n0=0):
    return np.zeros((h, w, 3)), np.zeros((h, w, 3)), np.full((h, w), n0, dtype=np.uint32)


@pytest.mark.parametrize("spp", [8, 5, 3])
@pytest.mark.parametrize("split", [1, 4, 8])
def test_both_forms_are_the_lane_code_bit_for_bit(libs, pk, frames, split, spp):
    """Spp 3 on 4 slots, 5 and 3 on 8: slots without a sample."""
    wf, lane = libs
    p = make_params(W, H, spp, BOUNCES, SEED, PT_FLAG_AA)
    a, wS, wQ = lane_code(lane, pk, p, split)
    got, steps, _ = wf_render(wf, pk, p, split)
    assert a.any() and same(got, a)
    per_slot = -(-spp // split)
    assert 2 < steps <= per_slot * (BOUNCES + 1) + 2
    S, Q, n, _, _ = wf_pass(wf, pk, p, ALL, (spp, spp, spp), split, *empty())
    assert same(S, wS) and same(Q, wQ) and (n == spp).all()
    want = frames[:spp]
    d = [float(np.abs(x - y).max()) for x, y in ((got, want.sum(axis=0)), (S, want.sum(axis=0)),
                                                 (Q, (want ** 2).sum(axis=0)))]
    print(f"split {split} spp {spp}: |sum|, |S|, |Q| vs oracle = {d}")
    assert max(d) <= 1e-12


def test_mixed_list_pass(libs, pk, frames):
    """One pass with pixels of unequal n and k (k = 3 from n = 0, k = 5 from
    n = 3) at 2 slots per entry, on a strict subset; an entry that is no pixel
    of the frame is skipped."""
    wf, lane = libs
    rs = np.random.RandomState(7)
    n0 = rs.choice(np.array([0, 3, 16], dtype=np.uint32), size=(H, W))
    S0 = np.where((n0 == 3)[..., None], frames[:3].sum(axis=0), 0.0) + (n0 == 16)[..., None] * 0.25
    Q0 = np.where((n0 == 3)[..., None], (frames[:3] ** 2).sum(axis=0), 0.0)
    lst = np.flatnonzero(rs.rand(W * H) < 0.4).astype(np.uint32)
    lst = lst[n0.ravel()[lst] < 16]
    assert 20 < len(lst) < W * H - 20 and (np.diff(lst) > 1).any()
    assert {0, 3} <= set(n0.ravel()[lst].tolist())
    rule = (3, 17, 5)
    S, Q, n, _, _ = wf_pass(wf, pk, make_params(W, H, 17, BOUNCES, SEED, PT_FLAG_AA),
                            np.append(lst, np.uint32(W * H + 5)), rule, 2, S0, Q0, n0)
    listed = np.zeros(W * H, dtype=bool)
    listed[lst] = True
    listed = listed.reshape(H, W)
    for got, was in ((S, S0), (Q, Q0), (n, n0)):
        assert np.array_equal(got[~listed], was[~listed])
    k = np.where(n0 < 3, 3, 5)
    assert np.array_equal(n[listed], (n0 + k)[listed])
    # the single kernel's list pass: the lane code of each pixel's own range
    _, s3, q3 = lane_code(lane, pk, make_params(W, H, 3, BOUNCES, SEED, PT_FLAG_AA), 2)
    _, s5, q5 = lane_code(lane, pk, make_params(W, H, 5, BOUNCES, SEED, PT_FLAG_AA, sample_begin=3), 2)
    first = (n0 == 0)[..., None]
    assert same(S[listed], (S0 + np.where(first, s3, s5))[listed])
    assert same(Q[listed], (Q0 + np.where(first, q3, q5))[listed])
    upto = np.where(listed, n0 + k, 0)
    wS = sum(frames[s] * (s < upto)[..., None] for s in range(8))
    wQ = sum(frames[s] ** 2 * (s < upto)[..., None] for s in range(8))
    assert np.abs(S - wS)[listed].max() <= 1e-12 and np.abs(Q - wQ)[listed].max() <= 1e-12


@pytest.mark.parametrize("case", ["rr", "no_bounces", "one_bounce"])
def test_other_paths(libs, pk, mesh_golden, case):
    wf, lane = libs
    flags, rr_depth, bounces = {"rr": (PT_FLAG_RR, 1, 4), "no_bounces": (0, 3, 0),
                                "one_bounce": (0, 3, 1)}[case]
    w = h = 8
    p = make_params(w, h, 4, bounces, SEED, PT_FLAG_AA | flags, rr_depth)
    want = None
    if bounces:
        want = aa_ref.to_image(aa_ref.aa_samples(mesh_golden[0], w, h, bounces, SEED, 4, flags=flags,
                                                 rr_depth=rr_depth), w, h)
    for split in (1, 4):
        a, wS, wQ = lane_code(lane, pk, p, split)
        got, steps, _ = wf_render(wf, pk, p, split)
        S, Q, n, lsteps, _ = wf_pass(wf, pk, p, np.arange(w * h), (4, 4, 4), split, *empty(h, w))
        assert same(got, a) and same(S, wS) and same(Q, wQ) and (n == 4).all()
        if bounces == 0:
            assert not got.any() and not S.any() and not Q.any()
            assert steps == 1 and lsteps == 1       # step 0 only: no slot ever starts
        else:
            assert got.any()
            assert np.abs(got - want.sum(axis=0)).max() <= 1e-12
            assert np.abs(Q - (want ** 2).sum(axis=0)).max() <= 1e-12


def test_drain_needs_the_primary_steps(libs, pk, frames):
    """A sample takes its primary query and then `bounces` bounce steps: every
    slot is done after per_slot (bounces + 1) + 2 shade steps, and at one slot
    per pixel some are still busy after the centre-ray form's bound."""
    wf, _ = libs
    for spp, split in ((8, 1), (8, 4), (5, 4)):
        per_slot = -(-spp // split)
        bound, centre = per_slot * (BOUNCES + 1) + 2, per_slot * BOUNCES + 2
        p = make_params(W, H, spp, BOUNCES, SEED, PT_FLAG_AA)
        _, steps, busy = wf_render(wf, pk, p, split)
        _, _, _, lsteps, lbusy = wf_pass(wf, pk, p, ALL, (spp, spp, spp), split, *empty())
        for s, b in ((steps, busy), (lsteps, lbusy)):
            print(f"spp {spp} split {split}: {s} steps of {bound}; busy after step {centre}: {b[centre - 1]}")
            assert s <= bound and b[s - 1] == 0 and (b[:s - 1] > 0).all()
            assert np.array_equal(busy[:s], b[:s])
            if split == 1:
                assert b[centre - 1] > 0      # the centre-ray step count would cut these paths


def test_stale_buffers(libs, pk):
    """The buffers hold another run's state (a wider launch of either form):
    step 0 initialises everything a run reads."""
    wf, _ = libs
    p = make_params(W, H, 5, BOUNCES, SEED, PT_FLAG_AA)
    other = make_params(W, H, 8, 2, 11, PT_FLAG_AA | PT_FLAG_RR, 0)
    clean = wf_render(wf, pk, p, 2)[0]
    clean_l = wf_pass(wf, pk, p, ALL, (5, 5, 5), 2, *empty())[:3]
    wf_pass(wf, pk, other, ALL, (8, 8, 8), 4, *empty())
    assert same(wf_render(wf, pk, p, 2, fresh=0)[0], clean)
    wf_render(wf, pk, other, 8)
    got = wf_pass(wf, pk, p, ALL, (5, 5, 5), 2, *empty(), fresh=0)[:3]
    assert same(got[0], clean_l[0]) and same(got[1], clean_l[1]) and np.array_equal(got[2], clean_l[2])
    assert same(wf_render(wf, pk, p, 2, fresh=0)[0], clean)
