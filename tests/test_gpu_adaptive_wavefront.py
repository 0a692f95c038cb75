"""Adaptive sampling on BVH scenes through the wavefront kernels (the list
form: pt_shade.h k_wf_shade_list, pt_hip.hip k_wf_primary_list /
k_wf_final_list, render_wavefront's list form): which path a pass takes,
whole runs and single passes against the single-kernel list pass
(megakernel=True) bit for bit and against the oracle's per-sample colours,
wide splits and ragged launches, the spilled walk stacks, and the buffers a
scene handle shares between its accumulators and uniform renders.  Host-side
cases: tests/test_adaptive_wavefront_host.py."""
import numpy as np
import pytest

from adaptive_sim import histogram, k_numpy, moments_upto, oracle_samples, simulate
from deep_scenes import COMB_ABOVE, COMB_BELOW, comb_scene, sliver_scene
from pathtracerpython_amd._abi import (PT_FLAG_FORCE_F64, PT_FLAG_KERNEL_TIMES, PT_FLAG_MEGAKERNEL,
                                       PT_FLAG_RR, PT_FLAG_WALK_COUNT, make_adapt, with_flags)
from pathtracerpython_amd.adaptive import Accumulator, run_passes
from pathtracerpython_amd.render import Renderer

pytestmark = pytest.mark.gpu

TOL = 1e-12
FLOOR = 0.01
MESH = (12, 12, 3, 5)      # W, H, bounces, seed
K5 = (10, 6, 3, 9)


@pytest.fixture(scope="module")
def mesh(mesh_golden):
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    with Renderer(mesh_golden[0]) as r:
        yield r


@pytest.fixture(scope="module")
def k5(k5mini_golden):
    with Renderer(k5mini_golden[0]) as r:
        yield r


@pytest.fixture(scope="module")
def mesh_frames(mesh):
    """Mesh scene 12x12, 3 bounces, seed 5: the oracle's 32 per-sample frames."""
    W, H, B, seed = MESH
    return oracle_samples(mesh.packed, W, H, B, seed, 32)


@pytest.fixture(scope="module")
def k5_frames(k5):
    W, H, B, seed = K5
    return oracle_samples(k5.packed, W, H, B, seed, 17)


def same_bits(a, b):
    return all(np.array_equal(a[k].view(np.uint64) if a[k].dtype == np.float64 else a[k],
                              b[k].view(np.uint64) if b[k].dtype == np.float64 else b[k])
               for k in ("S", "Q", "n"))


def run(r, frame, rule, tol, megakernel=False, **kw):
    """A whole adaptive run: (S, Q, n dict, passes)."""
    W, H, B, seed = frame
    mn, mx, st = rule
    p = r.params(W, H, mx, B, seed, megakernel=megakernel, **kw)
    with Accumulator(r, W, H) as acc:
        passes = run_passes(acc, p, make_adapt(tol, mx, mn, st, FLOOR))
        return acc.read(S=True, Q=True, n=True), passes


def one_pass_stats(r, frame, spp, flags):
    W, H, B, seed = frame
    p = with_flags(r.params(W, H, spp, B, seed), flags)
    with Accumulator(r, W, H) as acc:
        st = acc.render(p, make_adapt(0.0, spp, spp, spp), stats=True)
        return st, acc.read(S=True, Q=True, n=True)


# 1 ---------------------------------------------------------- the path ran --
def test_a_default_pass_runs_the_wavefront_kernels(mesh):
    st, d = one_pass_stats(mesh, MESH, 4, PT_FLAG_KERNEL_TIMES)
    assert st["shade_launches"] > 0 and st["shadow_launches"] > 0 and st["closest_launches"] > 0
    # 4 samples over 4 slots: one sample per slot, 3 bounces -> 5 shade steps, 4 walk steps
    assert st["shade_launches"] == 5 and st["shadow_launches"] == 4 and st["closest_launches"] == 4
    assert (d["n"] == 4).all()
    for flag in (PT_FLAG_MEGAKERNEL, PT_FLAG_FORCE_F64):
        st1, d1 = one_pass_stats(mesh, MESH, 4, PT_FLAG_KERNEL_TIMES | flag)
        assert st1["shade_launches"] == st1["shadow_launches"] == st1["closest_launches"] == 0
        assert (d1["n"] == 4).all()
        if flag == PT_FLAG_MEGAKERNEL:
            assert same_bits(d, d1)


@pytest.mark.parametrize("comb,wavefront", [(COMB_BELOW, True), (COMB_ABOVE, False)],
                         ids=["qstack48", "qstack49"])
def test_comb_scenes_at_the_walk_stack_bound(tmp_path, comb, wavefront):
    frame = (20, 16, 4, 9)
    with Renderer(comb_scene(tmp_path, *comb)) as r:
        st, d = one_pass_stats(r, frame, 2, PT_FLAG_KERNEL_TIMES)
        _, mk = one_pass_stats(r, frame, 2, PT_FLAG_MEGAKERNEL)
    launches = (st["shade_launches"], st["shadow_launches"], st["closest_launches"])
    assert all(n > 0 for n in launches) if wavefront else launches == (0, 0, 0)
    assert same_bits(d, mk)


# 2 ------------------------------------------------------------ whole runs --
RUNS = {(3, 17, 5): (0.05, {3: 67, 8: 8, 13: 5, 17: 64}, [144, 77, 69, 64], 1.86e-2),
        (4, 32, 4): (0.2, {4: 117, 8: 11, 12: 3, 16: 1, 20: 5, 24: 1, 32: 6},
                     [144, 27, 16, 13, 12, 7, 6, 6], 4.1e-3)}


def check_run(r, frame, frames, rule, tol, hist, lengths, margin):
    mn, mx, st = rule
    sim = simulate(frames[:mx], tol, FLOOR, mn, mx, st)
    print(f"rule {rule} tol {tol}: counts {histogram(sim['n'])}, "
          f"lists {[a for a, _ in sim['passes']]}, margin {sim['margin']:.3e}")
    assert histogram(sim["n"]) == hist
    assert [a for a, _ in sim["passes"]] == lengths
    assert 0.95 * margin <= sim["margin"] <= 1.05 * margin
    d, passes = run(r, frame, rule, tol)
    mk, passes_mk = run(r, frame, rule, tol, megakernel=True)
    assert same_bits(d, mk) and passes == passes_mk
    assert np.array_equal(d["n"], sim["n"]) and passes == sim["passes"]
    wS, wQ = moments_upto(frames, d["n"])
    dS, dQ = float(np.abs(d["S"] - wS).max()), float(np.abs(d["Q"] - wQ).max())
    print(f"|S - oracle| = {dS:.3e}, |Q - oracle| = {dQ:.3e}")
    assert dS <= TOL and dQ <= TOL


@pytest.mark.parametrize("rule", list(RUNS), ids=lambda r: "min%d_max%d_step%d" % r)
def test_mesh_runs_equal_the_single_kernel_and_the_oracle_simulation(mesh, mesh_frames, rule):
    check_run(mesh, MESH, mesh_frames, rule, *RUNS[rule])


def test_k5_generator_run(k5, k5_frames):
    check_run(k5, K5, k5_frames, (3, 17, 5), 0.1, {3: 44, 8: 6, 17: 10}, [60, 16, 10, 10], 7.9e-2)


# 3 ---------------------------------------------- mixed n and k in one pass --
def test_mixed_n_and_k_in_one_pass(mesh, mesh_frames):
    """After the (3, 17, 5) run the pixels hold n = 3, 8, 13, 17; one pass of
    rule (min 10, max 20, step 6, tol 0) adds k = 6, 2, 6, 3 (the step caps
    the 7 samples n = 3 lacks to min_spp): kmin = 2, two slots per entry with
    unequal shares, sample0 = n[e] + c differing between the entries of the
    pass."""
    W, H, B, seed = MESH
    out = {}
    for mkern in (False, True):
        with Accumulator(mesh, W, H) as acc:
            run_passes(acc, mesh.params(W, H, 17, B, seed, megakernel=mkern),
                       make_adapt(0.05, 17, 3, 5, FLOOR))
            n0 = acc.read(n=True)["n"]
            a2 = make_adapt(0.0, 20, 10, 6, FLOOR)
            assert acc.select(a2)[0] == W * H
            acc.render(mesh.params(W, H, 20, B, seed, megakernel=mkern), a2)
            out[mkern] = acc.read(S=True, Q=True, n=True)
    d = out[False]
    assert histogram(n0) == {3: 67, 8: 8, 13: 5, 17: 64}
    k = k_numpy(n0, 10, 20, 6)
    assert histogram(k) == {2: 8, 3: 64, 6: 72}
    assert np.array_equal(d["n"], n0 + k)
    assert same_bits(d, out[True])
    wS, wQ = moments_upto(mesh_frames, d["n"])
    assert np.abs(d["S"] - wS).max() <= TOL and np.abs(d["Q"] - wQ).max() <= TOL


# 4 --------------------------------------- wide splits and ragged launches --
@pytest.mark.parametrize("W,H,spp", [(5, 7, 16), (5, 7, 64), (1, 1, 16), (3, 1, 64)],
                         ids=lambda v: str(v))
def test_wide_splits_and_ragged_launches(mesh, W, H, spp):
    """5 x 7 at 64 slots per entry: 35 entries, 2,240 slots, the last block of
    256 partial; 1 x 1 and 3 x 1: less than one block."""
    frame = (W, H, 3, 5)
    d, passes = run(mesh, frame, (spp, spp, spp), 0.0)
    mk, _ = run(mesh, frame, (spp, spp, spp), 0.0, megakernel=True)
    assert passes == [(W * H, W * H * spp)] and (d["n"] == spp).all()
    assert same_bits(d, mk)
    assert d["S"].any() or W * H <= 3    # (the corner rays of the tiny frames miss the room)


# 5 ------------------------------------------------- RR and zero bounces --
def test_russian_roulette_and_no_bounces(k5):
    W, H, B, seed = K5
    d, _ = run(k5, K5, (8, 8, 8), 0.0, rr=True, rr_depth=1)
    mk, _ = run(k5, K5, (8, 8, 8), 0.0, megakernel=True, rr=True, rr_depth=1)
    c = oracle_samples(k5.packed, W, H, B, seed, 8, flags=PT_FLAG_RR, rr_depth=1)
    assert same_bits(d, mk) and (d["n"] == 8).all()
    assert np.abs(d["S"] - c.sum(axis=0)).max() <= TOL
    assert np.abs(d["Q"] - (c ** 2).sum(axis=0)).max() <= TOL
    d, passes = run(k5, (W, H, 0, seed), (3, 17, 5), 0.05)
    assert not d["S"].any() and not d["Q"].any()
    # n advances by k = 3; zero variance then stops every pixel at min_spp
    assert (d["n"] == 3).all() and passes == [(W * H, 3 * W * H)]


# 6 ----------------------------------------------------------- sliver scene --
def test_sliver_scene_through_the_spilled_stacks(tmp_path):
    frame = (16, 16, 4, 9)
    with Renderer(sliver_scene(tmp_path)) as r:
        d, _ = run(r, frame, (4, 4, 4), 0.0)
        mk, _ = run(r, frame, (4, 4, 4), 0.0, megakernel=True)
        st, dc = one_pass_stats(r, frame, 4, PT_FLAG_WALK_COUNT)
        c = oracle_samples(r.packed, 16, 16, 4, 9, 4)
    assert same_bits(d, mk) and same_bits(d, dc)
    dS = float(np.abs(d["S"] - c.sum(axis=0)).max())
    dQ = float(np.abs(d["Q"] - (c ** 2).sum(axis=0)).max())
    print(f"sliver list pass: |S - sum c| = {dS:.3e}, |Q - sum c^2| = {dQ:.3e}, walk counts "
          f"{ {k: v for k, v in st.items() if k.startswith(('shadow_', 'closest_')) and not k.endswith(('_ms', '_launches'))} }")
    assert dS <= TOL and dQ <= TOL
    assert st["shadow_queries"] > 0 and st["closest_queries"] > 0
    assert st["shadow_node_visits"] > 0 and st["closest_node_visits"] > 0


# 7 ---------------------------------------------------------- shared buffers --
def test_interleaved_accumulators_and_a_uniform_render_share_the_buffers(mesh):
    """Passes of two accumulators of different frame sizes on one Renderer,
    with a uniform wavefront render of a third size between them: the path
    slots, query records and moment home are the scene handle's, and every
    pass initialises what it uses."""
    fa, fb_, fu = (12, 12, 3, 5), (7, 5, 3, 11), (9, 4, 3, 5)
    rule, tol = (3, 17, 5), 0.05
    alone_a, pa = run(mesh, fa, rule, tol)
    alone_b, pb = run(mesh, fb_, rule, tol)
    alone_u = mesh.render(fu[0], fu[1], spp=6, bounces=fu[2], seed=fu[3], out_f64=True)
    adapt = make_adapt(tol, rule[1], rule[0], rule[2], FLOOR)
    pA = mesh.params(fa[0], fa[1], rule[1], fa[2], fa[3])
    pB = mesh.params(fb_[0], fb_[1], rule[1], fb_[2], fb_[3])
    with Accumulator(mesh, fa[0], fa[1]) as A, Accumulator(mesh, fb_[0], fb_[1]) as B:
        left = [A, B]
        uniform = []
        while left:
            for acc, p in ((A, pA), (B, pB)):
                if acc in left:
                    if acc.select(adapt)[0]:
                        acc.render(p, adapt)
                    else:
                        left.remove(acc)
                uniform.append(mesh.render(fu[0], fu[1], spp=6, bounces=fu[2], seed=fu[3], out_f64=True))
        da, db = A.read(S=True, Q=True, n=True), B.read(S=True, Q=True, n=True)
    assert len(pa) > 1 and len(pb) > 1 and len(uniform) >= 4
    assert same_bits(da, alone_a) and same_bits(db, alone_b)
    assert all(np.array_equal(u, alone_u) for u in uniform)
