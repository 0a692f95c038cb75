"""The walk kernels' spilled stacks and the deep-tree fallback on the GPU.

k_wf_shadow / k_wf_closest (pt_hip.hip) keep entries 0 .. 15 of a lane's walk
stack in shared memory and entries 16 .. 47 in a global overflow buffer
(render_wavefront's ovf_s / ovf_cr / ovf_cd, laid next to each other and to
the primary queries).  The sliver scene of tests/deep_scenes.py makes both
walks hold up to 21 entries, thousands of node visits of a 32 x 32 frame above
the shared-memory part (pinned on the host by tests/test_deep_bvh_host.py,
where the same split code runs on exactly sized heap blocks): a wrong stride,
an off-by-one at the split or a ref / dist mix-up in the overflow part changes
pixels here.  The single kernel, the forced-f64 render and the oracle are the
references; the walk kernels are under test.  The comb pair holds `qstack` 48
and 49: the last tree the walk kernels take and the first one the library must
hand to the single kernel."""
import numpy as np
import pytest

from adaptive_sim import oracle_samples
from deep_scenes import COMB_ABOVE, COMB_BELOW, COMB_FRAME, comb_scene, sliver_scene
from oracle import oracle
from pathtracerpython_amd._abi import PT_FLAG_RR, make_adapt
from pathtracerpython_amd.adaptive import Accumulator
from pathtracerpython_amd.render import Renderer, to_list_order

pytestmark = pytest.mark.gpu

TOL = 1e-12
# (W, H, spp, bounces, seed, rr): the frames tests/test_deep_bvh_host.py measures
FRAMES = [(32, 32, 2, 4, 9, False), (32, 32, 5, 3, 9, True)]


@pytest.fixture(scope="module")
def sliver(tmp_path_factory):
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    sc = sliver_scene(tmp_path_factory.mktemp("sliver"))
    with Renderer(sc) as r:
        yield r


def uniform_moments(r, W, H, spp, bounces, seed):
    """min = max = step = spp through the accumulator (k_render_list): (S, Q, n)."""
    adapt = make_adapt(0.0, spp, spp, spp)
    p = r.params(W, H, spp, bounces, seed)
    with Accumulator(r, W, H) as acc:
        while acc.select(adapt)[0]:
            acc.render(p, adapt)
        d = acc.read(S=True, Q=True, n=True)
    return d["S"], d["Q"], d["n"]


@pytest.mark.parametrize("W,H,spp,B,seed,rr", FRAMES, ids=["plain", "rr"])
def test_sliver_scene_through_the_spilled_stacks(sliver, W, H, spp, B, seed, rr):
    r = sliver
    wf, tt = r.render_params(r.params(W, H, spp, B, seed, rr=rr, out_f64=True, kernel_times=True),
                             stats=True)
    assert tt["shade_launches"] > 0                      # the wavefront path really ran
    assert tt["shadow_launches"] > 0 and tt["closest_launches"] > 0
    plain = r.render(W, H, spp, B, seed, rr=rr, out_f64=True)
    assert np.array_equal(plain, wf)
    mk = r.render(W, H, spp, B, seed, rr=rr, out_f64=True, megakernel=True)
    f64 = r.render(W, H, spp, B, seed, rr=rr, out_f64=True, force_f64=True)
    n_mk = int((wf != mk).any(axis=2).sum())
    n_64 = int((wf != f64).any(axis=2).sum())
    ref, _ = oracle.render(r.packed, W, H, spp, B, seed, flags=PT_FLAG_RR if rr else 0)
    d = float(np.abs(to_list_order(wf) - ref).max())
    print(f"sliver {W}x{H} spp {spp} B {B} rr {rr}: pixels != single kernel {n_mk}, "
          f"!= forced f64 {n_64}, |wavefront - oracle| = {d:.3e}")
    assert np.array_equal(wf, mk)
    assert np.array_equal(wf, f64)
    assert d <= TOL                                      # all 1,024 pixels
    band = r.render(W, H, spp, B, seed, rr=rr, out_f64=True, row_begin=5, row_end=29)
    assert np.array_equal(band, wf[H - 29:H - 5])
    fb, st = r.render_params(r.params(W, H, spp, B, seed, rr=rr, out_f64=True, walk_count=True),
                             stats=True)
    assert np.array_equal(fb, wf)                        # the counting walk kernels
    assert st["shadow_queries"] > 0 and st["closest_queries"] > 0
    assert st["shadow_node_visits"] > 0 and st["closest_node_visits"] > 0


def test_sliver_scene_through_the_list_kernel(sliver):
    W = H = 16
    S, Q, n = uniform_moments(sliver, W, H, 4, 4, 9)
    c = oracle_samples(sliver.packed, W, H, 4, 9, 4)
    dS = float(np.abs(S - c.sum(axis=0)).max())
    dQ = float(np.abs(Q - (c ** 2).sum(axis=0)).max())
    print(f"sliver list kernel: |S - sum c| = {dS:.3e}, |Q - sum c^2| = {dQ:.3e}")
    assert (n == 4).all()
    assert dS <= TOL and dQ <= TOL


def _comb(tmp_path, comb):
    W, H, spp, B, seed = COMB_FRAME
    with Renderer(comb_scene(tmp_path, *comb)) as r:
        fb, tt = r.render_params(r.params(W, H, spp, B, seed, out_f64=True, kernel_times=True),
                                 stats=True)
        assert np.array_equal(fb, r.render(W, H, spp, B, seed, out_f64=True))
        mk = r.render(W, H, spp, B, seed, out_f64=True, megakernel=True)
        f64 = r.render(W, H, spp, B, seed, out_f64=True, force_f64=True)
        ref, _ = oracle.render(r.packed, W, H, spp, B, seed)
    d = float(np.abs(to_list_order(fb) - ref).max())
    print(f"comb {comb}: shade launches {tt['shade_launches']}, |default - oracle| = {d:.3e}")
    assert np.array_equal(fb, mk)
    assert np.array_equal(fb, f64)
    assert d <= TOL
    return tt


def test_comb_below_the_bound_takes_the_walk_kernels(tmp_path):
    tt = _comb(tmp_path, COMB_BELOW)      # qstack 48 = kWalkStack
    assert tt["shade_launches"] > 0 and tt["shadow_launches"] > 0 and tt["closest_launches"] > 0


def test_comb_above_the_bound_takes_the_single_kernel(tmp_path):
    tt = _comb(tmp_path, COMB_ABOVE)      # qstack 49
    assert tt["shade_launches"] == 0 and tt["shadow_launches"] == 0 and tt["closest_launches"] == 0
