"""The walk kernels' split stacks and the deep-tree fallback, on the host.

k_wf_shadow / k_wf_closest (pt_hip.hip) keep stack entries 0 .. 15 in shared
memory and 16 .. 47 in a global overflow buffer; pt_path.h's ShadowStackT /
ClosestStackT and the `top + 3 <= nl` switch of push3 / push3_ref exist for
that split.  hc_render_wavefront3 (tests/hostcheck) runs the same walks on two
exactly sized heap blocks, so the split code runs here: it must reproduce the
local-stack framebuffer bit for bit wherever the split lies.  The sliver scene
of tests/deep_scenes.py is what makes the walks hold more than 16 entries;
test_sliver_scene_fills_the_walk_stacks pins that, as the premise of
tests/test_gpu_deep_bvh.py.  The comb pair holds `qstack` on either side of
kWalkStack = 48, the bound past which the library takes the single kernel."""
import ctypes as C

import numpy as np
import pytest

from conftest import hc_render
from deep_scenes import (COMB_ABOVE, COMB_BELOW, COMB_FRAME, WALK_STACK, WALK_STACK_LDS, comb_scene,
                         sliver_scene)
from oracle import oracle
from pathtracerpython_amd._abi import PT_FLAG_RR, make_params
from pathtracerpython_amd.pack import pack_scene
from pathtracerpython_amd.render import to_list_order

TOL = 1e-12
# the frames of tests/test_gpu_deep_bvh.py: (W, H, spp, bounces, seed, flags)
FRAMES = {"plain": (32, 32, 2, 4, 9, 0), "rr": (32, 32, 5, 3, 9, PT_FLAG_RR)}


def bvh_info(lib, pk):
    """dict(n_bnode, bvh_depth, n_qnode, qstack, n_bunitc, bvh_obj1)"""
    out = (C.c_int32 * 6)()
    assert lib.hc_bvh_info(C.byref(pk.desc), out) == 0
    return dict(zip(("n_bnode", "bvh_depth", "n_qnode", "qstack", "n_bunitc", "bvh_obj1"), out))


def wavefront3(lib, pk, p, lds_entries):
    """(rc, framebuffer, peak[4], walk_stats[8]) of hc_render_wavefront3."""
    out = np.zeros((p.height, p.width, 3))
    peak = (C.c_int64 * 4)()
    ws = (C.c_int64 * 8)()
    lib.hc_render_wavefront3.restype = C.c_int
    rc = lib.hc_render_wavefront3(C.byref(pk.desc), C.byref(p),
                                  out.ctypes.data_as(C.POINTER(C.c_double)), None, ws, None,
                                  C.c_int32(lds_entries), peak)
    return rc, out, list(peak), list(ws)


@pytest.fixture(scope="module")
def sliver(tmp_path_factory):
    return pack_scene(sliver_scene(tmp_path_factory.mktemp("sliver")))


@pytest.fixture(scope="module")
def local(hostcheck, sliver):
    """The sliver frames on the local stacks: {name: (framebuffer, peak, walk_stats)}."""
    out = {}
    for name, (W, H, spp, B, seed, flags) in FRAMES.items():
        rc, fb, peak, ws = wavefront3(hostcheck, sliver, make_params(W, H, spp, B, seed, flags), 0)
        assert rc == 0
        out[name] = (fb, peak, ws)
    return out


def test_sliver_scene_fills_the_walk_stacks(hostcheck, sliver, local):
    """Conditions on the input of the GPU tests, not tolerances: both walks
    reach kWalkStackLds + 4 entries (past push3's switch at 14 and past the
    first global entries), a thousand node visits of each leave more than 16,
    and the tree is within the walk kernels' 48 (the wavefront path takes it).
    Measured: peak 21 / 21, 5,988 / 1,903 visits above 16, qstack 26."""
    info = bvh_info(hostcheck, sliver)
    print("sliver scene:", info)
    assert info["n_qnode"] > 0 and info["qstack"] <= WALK_STACK
    for name, (_, peak, _) in local.items():
        print(f"{name}: peak top shadow / closest {peak[0]} / {peak[1]}, "
              f"node visits with top > 16: {peak[2]} / {peak[3]}")
        assert peak[0] >= WALK_STACK_LDS + 4 and peak[1] >= WALK_STACK_LDS + 4
        assert peak[2] >= 1000 and peak[3] >= 1000
        assert max(peak[0], peak[1]) <= info["qstack"]   # qstack bounds the entries held


@pytest.mark.parametrize("lds_entries", [16, 13, 3, 1])
def test_split_stacks_equal_local(hostcheck, sliver, local, lds_entries):
    """16: the GPU's split.  13: the switch of push3 not on a multiple of
    three.  3: nearly every push takes the slow branch.  1: nearly the whole
    stack in the global part."""
    W, H, spp, B, seed, flags = FRAMES["plain"]
    rc, fb, peak, ws = wavefront3(hostcheck, sliver, make_params(W, H, spp, B, seed, flags),
                                  lds_entries)
    assert rc == 0
    assert ws == local["plain"][2]               # as many rays, node visits, leaves
    assert peak == local["plain"][1]            # the same walks
    assert np.array_equal(fb, local["plain"][0])


@pytest.mark.parametrize("lds_entries", [16, 3])
def test_split_stacks_equal_local_russian_roulette(hostcheck, sliver, local, lds_entries):
    W, H, spp, B, seed, flags = FRAMES["rr"]
    rc, fb, peak, ws = wavefront3(hostcheck, sliver, make_params(W, H, spp, B, seed, flags),
                                  lds_entries)
    assert rc == 0
    assert ws == local["rr"][2]               # as many rays, node visits, leaves
    assert peak == local["rr"][1]
    assert np.array_equal(fb, local["rr"][0])


def test_split_argument_is_checked(hostcheck, sliver):
    p = make_params(4, 4, 1, 1, 1)
    assert wavefront3(hostcheck, sliver, p, -1)[0] == -4
    assert wavefront3(hostcheck, sliver, p, WALK_STACK + 1)[0] == -4
    assert wavefront3(hostcheck, sliver, p, WALK_STACK)[0] == 0   # no global part at all


@pytest.mark.parametrize("name", list(FRAMES))
def test_sliver_local_stacks_match_the_oracle(hostcheck, sliver, local, name):
    W, H, spp, B, seed, flags = FRAMES[name]
    ref, _ = oracle.render(sliver, W, H, spp, B, seed, flags)
    d = float(np.abs(to_list_order(local[name][0]) - ref).max())
    print(f"sliver {name}: |host wavefront - oracle| = {d:.3e}")
    assert d <= TOL
    single, _ = hc_render(hostcheck, sliver, make_params(W, H, spp, B, seed, flags), False,
                          count=False)
    assert np.array_equal(local[name][0], single)   # wavefront == single-kernel lane code


# ------------------------------------------------------------ fallback --
def _single_kernel_vs_oracle(lib, pk, W, H, spp, B, seed):
    p = make_params(W, H, spp, B, seed)
    a, _ = hc_render(lib, pk, p, False, count=False)
    b, _ = hc_render(lib, pk, p, True, count=False)
    ref, _ = oracle.render(pk, W, H, spp, B, seed)
    da = float(np.abs(to_list_order(a) - ref).max())
    db = float(np.abs(to_list_order(b) - ref).max())
    print(f"|hybrid - oracle| = {da:.3e}, |forced f64 - oracle| = {db:.3e}")
    assert da <= TOL and db <= TOL
    return a


def test_comb_frame_holds_no_exact_tie():
    """A condition on the input: no primary ray of the comb frame lies in a
    plane where the reference's own arithmetic ties (deep_scenes.COMB_FRAME).
    The frames that showed the ties must be refused."""
    from deep_scenes import comb_frame_is_generic
    assert comb_frame_is_generic(*COMB_FRAME[:2])
    assert not comb_frame_is_generic(20, 20)    # anti-diagonal rays in x + y = 0
    assert not comb_frame_is_generic(20, 17)    # centre row y = 0
    assert not comb_frame_is_generic(21, 16)    # centre column x = 0


def test_comb_below_the_bound_renders_through_the_walks(hostcheck, tmp_path):
    pk = pack_scene(comb_scene(tmp_path, *COMB_BELOW))
    info = bvh_info(hostcheck, pk)
    print("COMB_BELOW:", info)
    assert info["n_qnode"] > 0 and info["qstack"] <= WALK_STACK
    W, H, spp, B, seed = COMB_FRAME
    single = _single_kernel_vs_oracle(hostcheck, pk, W, H, spp, B, seed)
    p = make_params(W, H, spp, B, seed)
    for lds_entries in (0, WALK_STACK_LDS):
        rc, fb, _, _ = wavefront3(hostcheck, pk, p, lds_entries)
        assert rc == 0
        assert np.array_equal(fb, single)
    out = np.zeros((H, W, 3))
    steps = C.c_int32(0)
    assert hostcheck.hc_render_wavefront(C.byref(pk.desc), C.byref(p),
                                         out.ctypes.data_as(C.POINTER(C.c_double)),
                                         C.byref(steps), None) == 0
    assert np.array_equal(out, single)
    assert 1 <= steps.value <= spp * B + 2


def test_comb_above_the_bound_is_refused_by_the_walks(hostcheck, tmp_path):
    pk = pack_scene(comb_scene(tmp_path, *COMB_ABOVE))
    info = bvh_info(hostcheck, pk)
    print("COMB_ABOVE:", info)
    assert info["n_qnode"] > 0 and info["qstack"] > WALK_STACK
    W, H, spp, B, seed = COMB_FRAME
    _single_kernel_vs_oracle(hostcheck, pk, W, H, spp, B, seed)
    p = make_params(W, H, spp, B, seed)
    out = np.zeros((H, W, 3))
    assert hostcheck.hc_render_wavefront(C.byref(pk.desc), C.byref(p),
                                         out.ctypes.data_as(C.POINTER(C.c_double)), None,
                                         None) == -3
    assert wavefront3(hostcheck, pk, p, WALK_STACK_LDS)[0] == -3
