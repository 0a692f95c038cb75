"""The list form of the wavefront render on the host (pt_wavefront.h wf_shade
with the WfMoments home; tests/hostcheck/pt_accum_wf_host.cpp): one
accumulator pass over an active list through the slot state machine, against
the single kernel's lane code (hc_render_moments) bit for bit at split 1 and
against the oracle's per-sample colours at wider splits.  The GPU cases are
tests/test_gpu_adaptive_wavefront.py."""
import ctypes as C

import numpy as np
import pytest

import hostlib
from adaptive_sim import moments_upto, oracle_samples

from pathtracerpython_amd._abi import PT_FLAG_RR, make_params
from pathtracerpython_amd.pack import pack_scene

_dp = C.POINTER(C.c_double)
_up = C.POINTER(C.c_uint32)

W = H = 12
BOUNCES, SEED = 3, 5


@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    """pt_accum_wf_host.cpp (the list pass) and pt_accum_host.cpp (the single
    kernel's lane code), built as tests/test_adaptive.py builds the latter."""
    tmp = tmp_path_factory.mktemp("accum_wf_host")
    wf, mk = hostlib.build(tmp, "pt_accum_wf_host"), hostlib.build(tmp, "pt_accum_host")
    wf.hc_accum_wf_pass.restype = C.c_int
    wf.hc_accum_wf_pass.argtypes = [C.c_void_p, C.c_void_p, _up, C.c_uint32, C.c_uint32, C.c_uint32,
                                    C.c_uint32, C.c_uint32, _dp, _dp, _up, C.POINTER(C.c_int32)]
    mk.hc_render_moments.restype = C.c_int
    return wf, mk


@pytest.fixture(scope="module")
def mesh_packed(mesh_golden):
    return pack_scene(mesh_golden[0])


@pytest.fixture(scope="module")
def frames(mesh_packed):
    """Mesh scene 12x12, 3 bounces, seed 5: the oracle's 8 per-sample frames."""
    return oracle_samples(mesh_packed, W, H, BOUNCES, SEED, 8)


def list_pass(lib, packed, p, lst, rule, split, S, Q, n):
    """One pass over lst on copies of S, Q, n: (S, Q, n, shade steps)."""
    S, Q, n = S.copy(), Q.copy(), n.copy()
    lst = np.ascontiguousarray(lst, dtype=np.uint32)
    steps = C.c_int32(0)
    rc = lib.hc_accum_wf_pass(C.byref(packed.desc), C.byref(p), lst.ctypes.data_as(_up), len(lst),
                              *rule, split, S.ctypes.data_as(_dp), Q.ctypes.data_as(_dp),
                              n.ctypes.data_as(_up), C.byref(steps))
    assert rc == 0
    return S, Q, n, steps.value


def lane_moments(lib, packed, p):
    S = np.zeros((p.height, p.width, 3))
    Q = np.zeros((p.height, p.width, 3))
    n = np.zeros((p.height, p.width), dtype=np.uint32)
    rc = lib.hc_render_moments(C.byref(packed.desc), C.byref(p), 0, 0, S.ctypes.data_as(_dp),
                               Q.ctypes.data_as(_dp), n.ctypes.data_as(_up))
    assert rc == 0
    return S, Q, n


def empty(n0=0):
    return (np.zeros((H, W, 3)), np.zeros((H, W, 3)), np.full((H, W), n0, dtype=np.uint32))


# n = 3 everywhere, rule (min 3, max 17, step 5): every listed pixel takes k = 5
RULE = (3, 17, 5)
ALL = np.arange(W * H, dtype=np.uint32)


@pytest.mark.parametrize("case", ["plain", "rr", "no_bounces"])
def test_split_one_is_the_single_kernels_lane_code_bit_for_bit(libs, mesh_packed, case):
    wf, mk = libs
    flags, rr_depth = (PT_FLAG_RR, 1) if case == "rr" else (0, 3)
    bounces = 0 if case == "no_bounces" else BOUNCES
    p = make_params(W, H, 17, bounces, SEED, flags, rr_depth)
    S, Q, n, steps = list_pass(wf, mesh_packed, p, ALL, RULE, 1, *empty(3))
    want = lane_moments(mk, mesh_packed, make_params(W, H, 5, bounces, SEED, flags, rr_depth,
                                                     sample_begin=3))
    assert np.array_equal(S.view(np.uint64), want[0].view(np.uint64))
    assert np.array_equal(Q.view(np.uint64), want[1].view(np.uint64))
    assert (n == 8).all() and (want[2] == 5).all()
    if case == "no_bounces":
        assert not S.any() and not Q.any()
        assert steps == 1                       # step 0 only: no slot ever starts
    else:
        assert S.any() and 2 < steps <= 5 * bounces + 2


@pytest.mark.parametrize("split", [2, 8])
def test_wider_splits_match_the_oracle_per_sample(libs, mesh_packed, frames, split):
    """k = 5 over 2 slots (3 + 2 samples) and over 8 (slots 5..7 get none),
    from sample 3 on, on top of the oracle's first 3 samples."""
    wf, _ = libs
    n0 = np.full((H, W), 3, dtype=np.uint32)
    S0, Q0 = moments_upto(frames, n0)
    p = make_params(W, H, 17, BOUNCES, SEED)
    S, Q, n, _ = list_pass(wf, mesh_packed, p, ALL, RULE, split, S0, Q0, n0)
    wS, wQ = moments_upto(frames, np.full((H, W), 8))
    dS, dQ = float(np.abs(S - wS).max()), float(np.abs(Q - wQ).max())
    print(f"split {split}: |S - oracle| = {dS:.3e}, |Q - oracle| = {dQ:.3e}")
    assert (n == 8).all()
    assert dS <= 1e-12 and dQ <= 1e-12


def test_a_strict_subset_leaves_unlisted_pixels_untouched(libs, mesh_packed, frames):
    """A non-contiguous list with mixed n (k = 3 from n = 0, k = 5 from n = 3)
    at split 2; an entry that is no pixel of the frame is skipped."""
    wf, _ = libs
    rs = np.random.RandomState(7)
    n0 = rs.choice(np.array([0, 3, 16], dtype=np.uint32), size=(H, W))
    S0, Q0 = moments_upto(frames[:3], np.minimum(n0, 3))
    S0 = S0 + (n0 == 16)[..., None] * 0.25      # (any value: only the listed pixels' matter)
    lst = np.flatnonzero(rs.rand(W * H) < 0.4).astype(np.uint32)
    lst = lst[n0.ravel()[lst] < 16]              # keep the oracle frames in range: n + k <= 8
    assert 20 < len(lst) < W * H - 20 and (np.diff(lst) > 1).any()
    S, Q, n, _ = list_pass(wf, mesh_packed, make_params(W, H, 17, BOUNCES, SEED),
                           np.append(lst, np.uint32(W * H + 5)), RULE, 2, S0, Q0, n0)
    listed = np.zeros(W * H, dtype=bool)
    listed[lst] = True
    listed = listed.reshape(H, W)
    for got, was in ((S, S0), (Q, Q0), (n, n0)):
        assert np.array_equal(got[~listed], was[~listed])
    k = np.where(n0 < 3, 3, 5)
    assert np.array_equal(n[listed], (n0 + k)[listed])
    wS, wQ = moments_upto(frames, np.where(listed, n0 + k, 0))
    assert np.abs(S - wS)[listed].max() <= 1e-12 and np.abs(Q - wQ)[listed].max() <= 1e-12
