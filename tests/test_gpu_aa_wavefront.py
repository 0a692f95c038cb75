"""Antialiasing on BVH scenes through the wavefront kernels (pt_shade.h
k_wf_shade_aa / k_wf_shade_list_aa: a primary query per sample in the slot's
own record; render_wavefront with PT_FLAG_AA): which path a launch takes, the
frames and accumulator passes against the single kernel (megakernel=True) bit
for bit and against the oracle's antialiased per-sample colours
(tests/aa_ref.py), splits and ragged launches, sample ranges, bands, larger
trees, the buffers a scene handle shares, validation and the command line.
Host-side cases: tests/test_aa_wavefront_host.py."""
import os
import sys

import numpy as np
import pytest

import aa_ref
from adaptive_sim import histogram, k_numpy, simulate
from conftest import CORNELL, GOLDEN
from deep_scenes import COMB_ABOVE, COMB_BELOW, comb_scene, sliver_scene
from pathtracerpython_amd import _native
from pathtracerpython_amd._abi import (PT_FLAG_AA, PT_FLAG_COUNT, PT_FLAG_FORCE_F64, PT_FLAG_KERNEL_TIMES,
                                       PT_FLAG_MEGAKERNEL, PT_FLAG_RR, PT_FLAG_WALK_COUNT, make_adapt,
                                       with_flags)
from pathtracerpython_amd.adaptive import Accumulator, render_adaptive, render_adaptive_multi, run_passes
from pathtracerpython_amd.progressive import render_progressive
from pathtracerpython_amd.render import MultiRenderer, Renderer

pytestmark = pytest.mark.gpu

TOL = 1e-12
FLOOR = 0.01
MESH = (12, 12, 3, 5)      # W, H, bounces, seed
REFUSED = r"\(-1\): .*PT_FLAG_AA does not combine"


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else a.dtype)


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def same_bits(a, b):
    return all(same(a[k], b[k]) for k in ("S", "Q", "n"))


@pytest.fixture(scope="module")
def mesh(mesh_golden):
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    with Renderer(mesh_golden[0]) as r:
        yield r


def covered(c, light_rgb, need=3):
    """The frame runs the branches of the restart: mixed-escape, mixed-light
    (and all-escape, need = 3) pixels."""
    cov = aa_ref.coverage(c, light_rgb)
    print(f"coverage {cov}")
    assert min(cov[:need]) >= 1
    return c


@pytest.fixture(scope="module")
def ref12(mesh_golden, mesh):
    """Mesh scene 12x12, 3 bounces, seed 5: the oracle's 17 antialiased
    per-sample frames, image orientation; the first 8 and the first 2 of them
    run every branch of the restart."""
    c = aa_ref.aa_samples(mesh_golden[0], 12, 12, 3, 5, 17)
    covered(c[:8], mesh.packed.light_rgb)
    covered(c[:2], mesh.packed.light_rgb)
    return aa_ref.to_image(c, 12, 12)


@pytest.fixture(scope="module")
def ref75(mesh_golden):
    return aa_ref.to_image(aa_ref.aa_samples(mesh_golden[0], 7, 5, 3, 5, 8), 7, 5)


def mean_err(fb, ref, spp, begin=0):
    return float(np.abs(fb - ref[begin:begin + spp].sum(axis=0) / spp).max())


def both(r, *a, **kw):
    """(wavefront, single kernel) frames of one antialiased render."""
    return (r.render(*a, out_f64=True, aa=True, **kw), r.render(*a, out_f64=True, aa=True, megakernel=True, **kw))


def one_pass(r, frame, spp, flags, stats=True):
    W, H, B, seed = frame
    p = with_flags(r.params(W, H, spp, B, seed), flags)
    with Accumulator(r, W, H) as acc:
        st = acc.render(p, make_adapt(0.0, spp, spp, spp), stats=stats)
        return st, acc.read(S=True, Q=True, n=True)


def run(r, frame, rule, tol, megakernel=False, **kw):
    """A whole antialiased adaptive run: (S, Q, n dict, passes)."""
    W, H, B, seed = frame
    mn, mx, st = rule
    p = r.params(W, H, mx, B, seed, megakernel=megakernel, aa=True, **kw)
    with Accumulator(r, W, H) as acc:
        passes = run_passes(acc, p, make_adapt(tol, mx, mn, st, FLOOR))
        return acc.read(S=True, Q=True, n=True), passes


# 1 ---------------------------------------------------------- the path ran --
def test_an_antialiased_pass_runs_the_wavefront_kernels(mesh):
    """4 samples over 4 slots, 3 bounces: a sample is its primary query and
    three bounce steps, so 1 x (3 + 1) + 2 shade steps and one walk step less."""
    st, d = one_pass(mesh, MESH, 4, PT_FLAG_AA | PT_FLAG_KERNEL_TIMES)
    assert (st["shade_launches"], st["shadow_launches"], st["closest_launches"]) == (6, 5, 5)
    assert (d["n"] == 4).all()
    _, mk = one_pass(mesh, MESH, 4, PT_FLAG_AA | PT_FLAG_MEGAKERNEL, stats=False)
    assert same_bits(d, mk)
    for flag in (PT_FLAG_MEGAKERNEL, PT_FLAG_FORCE_F64):
        with pytest.raises(_native.NativeError, match=REFUSED):
            one_pass(mesh, MESH, 4, PT_FLAG_AA | PT_FLAG_KERNEL_TIMES | flag)


def test_an_antialiased_render_runs_the_wavefront_kernels(mesh):
    W, H, B, seed = MESH
    p = mesh.params(W, H, 4, B, seed, out_f64=True, aa=True, kernel_times=True, lanes_per_pixel=4)
    fb, st = mesh.render_params(p, stats=True)
    assert (st["shade_launches"], st["shadow_launches"], st["closest_launches"]) == (6, 5, 5)
    assert same(fb, mesh.render(W, H, 4, B, seed, out_f64=True, aa=True, megakernel=True, lanes_per_pixel=4))
    for flag in (PT_FLAG_MEGAKERNEL, PT_FLAG_FORCE_F64):
        with pytest.raises(_native.NativeError, match=REFUSED):
            mesh.render_params(with_flags(p, flag), stats=True)


@pytest.mark.parametrize("comb,wavefront", [(COMB_BELOW, True), (COMB_ABOVE, False)],
                         ids=["qstack48", "qstack49"])
def test_comb_scenes_at_the_walk_stack_bound(tmp_path, comb, wavefront):
    frame = (20, 16, 4, 9)
    with Renderer(comb_scene(tmp_path, *comb)) as r:
        _, d = one_pass(r, frame, 2, PT_FLAG_AA, stats=False)
        _, mk = one_pass(r, frame, 2, PT_FLAG_AA | PT_FLAG_MEGAKERNEL, stats=False)
        assert same_bits(d, mk) and d["S"].any()
        if wavefront:
            st, dt = one_pass(r, frame, 2, PT_FLAG_AA | PT_FLAG_KERNEL_TIMES)
            assert st["shade_launches"] > 0 and st["shadow_launches"] > 0 and st["closest_launches"] > 0
            assert same_bits(d, dt)
        else:       # the single kernel: the flag is refused, as on a scene without a BVH
            with pytest.raises(_native.NativeError, match=REFUSED):
                one_pass(r, frame, 2, PT_FLAG_AA | PT_FLAG_KERNEL_TIMES)
            with pytest.raises(_native.NativeError, match=REFUSED):
                r.render_params(r.params(20, 16, 2, 4, 9, aa=True, walk_count=True), stats=True)
            a, b = both(r, 20, 16, 2, 4, 9)
            assert same(a, b)


# 2 ------------------------------------------------------------------ frames --
@pytest.mark.parametrize("spp", [2, 8])
def test_frames(mesh, ref12, spp):
    W, H, B, seed = MESH
    fb, mk = both(mesh, W, H, spp, B, seed)
    assert same(fb, mk)
    e = mean_err(fb, ref12, spp)
    print(f"12x12x{spp} antialiased wavefront frame vs oracle: {e:.3e}")
    assert e <= TOL
    f32 = mesh.render(W, H, spp, B, seed, aa=True)
    assert f32.dtype == np.float32 and mean_err(f32.astype(np.float64), ref12, spp) <= 1e-6
    assert np.abs(fb - mesh.render(W, H, spp, B, seed, out_f64=True)).max() > 1e-3   # not the centre ray


# 3 ------------------------------------------------ splits, ragged launches --
@pytest.mark.parametrize("lanes", [1, 2, 4])
def test_slots_per_pixel(mesh, ref75, lanes):
    """7 x 5 at 8 / 5 / 3 samples (4 slots need 4 samples: lanes_per_pixel <=
    spp); 5 samples on 4 slots: unequal shares."""
    for spp in (8, 5, 3):
        if lanes > spp:
            continue
        fb, mk = both(mesh, 7, 5, spp, 3, 5, lanes_per_pixel=lanes)
        assert fb.shape == (5, 7, 3) and same(fb, mk)
        assert mean_err(fb, ref75, spp) <= TOL


@pytest.mark.parametrize("lanes", [16, 64])
def test_wide_pixels(mesh, mesh_golden, lanes):
    c = covered(aa_ref.aa_samples(mesh_golden[0], 6, 6, 2, 5, 64), mesh.packed.light_rgb, need=2)
    fb, mk = both(mesh, 6, 6, 64, 2, 5, lanes_per_pixel=lanes)
    assert same(fb, mk)
    assert mean_err(fb, aa_ref.to_image(c, 6, 6), 64) <= TOL


@pytest.mark.parametrize("W,H", [(5, 7), (1, 1), (3, 1)])
def test_partial_last_shade_block(mesh, W, H):
    for lanes in (1, 4):
        fb, mk = both(mesh, W, H, 4, 3, 5, lanes_per_pixel=lanes)
        assert fb.shape == (H, W, 3) and same(fb, mk)


# 4 ----------------------------------------- RR, zero bounces, one bounce --
def test_russian_roulette_no_bounces_and_one_bounce(mesh, mesh_golden):
    ref = aa_ref.to_image(aa_ref.aa_samples(mesh_golden[0], 12, 12, 4, 5, 8, flags=PT_FLAG_RR, rr_depth=1),
                          12, 12)
    fb, mk = both(mesh, 12, 12, 8, 4, 5, rr=True, rr_depth=1)
    assert same(fb, mk) and mean_err(fb, ref, 8) <= TOL
    fb, mk = both(mesh, 12, 12, 8, 0, 5)
    assert same(fb, mk) and not fb.any()
    ref = aa_ref.to_image(aa_ref.aa_samples(mesh_golden[0], 12, 12, 1, 5, 8), 12, 12)
    fb, mk = both(mesh, 12, 12, 8, 1, 5)
    assert same(fb, mk) and fb.any() and mean_err(fb, ref, 8) <= TOL
    for b in (0, 1):
        _, d = one_pass(mesh, (12, 12, b, 5), 4, PT_FLAG_AA, stats=False)
        _, m = one_pass(mesh, (12, 12, b, 5), 4, PT_FLAG_AA | PT_FLAG_MEGAKERNEL, stats=False)
        assert same_bits(d, m) and (d["n"] == 4).all()


# 5 ------------------------------------------------ sample ranges, chunks --
def test_sample_ranges_and_chunks(mesh, ref12, tmp_path):
    W, H, B, seed = MESH
    fb, mk = both(mesh, W, H, 3, B, seed, sample_begin=5)
    assert same(fb, mk) and mean_err(fb, ref12, 3, begin=5) <= TOL
    one = mesh.render(W, H, 8, B, seed, out_f64=True, aa=True)
    two = render_progressive(mesh, W, H, 8, B, seed, chunk_spp=4, aa=True)
    assert np.abs(two - one).max() <= 1e-14
    ck = str(tmp_path / "aa.npz")
    assert render_progressive(mesh, W, H, 8, B, seed, chunk_spp=4, checkpoint=ck, max_chunks=1,
                              aa=True) is None
    assert same(render_progressive(mesh, W, H, 8, B, seed, chunk_spp=4, checkpoint=ck, aa=True), two)


# 6 ------------------------------------------------------------------- bands --
def test_bands_equal_the_whole_frame_bit_for_bit(mesh):
    import torch
    W, H, spp = 7, 5, 8
    whole = mesh.render(W, H, spp, 3, 5, out_f64=True, aa=True, lanes_per_pixel=4)
    s = torch.cuda.current_stream().cuda_stream
    frame = torch.full((H, W, 3), float("nan"), dtype=torch.float64, device="cuda")
    for phase in range(2):      # interleaved rows, both phases
        iy_top = max(range(phase, H, 2))
        p = mesh.params(W, H, spp, 3, 5, out_f64=True, aa=True, lanes_per_pixel=4, row_step=2,
                        row_phase=phase, out_row_stride=2 * W * 3)
        mesh.render_device(p, frame[H - 1 - iy_top].data_ptr(), s)
    torch.cuda.synchronize()
    assert same(frame.cpu().numpy(), whole)
    frame = torch.full((H, W, 3), float("nan"), dtype=torch.float64, device="cuda")
    for rb, re in ((0, 2), (2, 5)):      # a contiguous split
        p = mesh.params(W, H, spp, 3, 5, out_f64=True, aa=True, lanes_per_pixel=4, row_begin=rb,
                        row_end=re, out_row_stride=W * 3)
        mesh.render_device(p, frame[H - re].data_ptr(), s)
    torch.cuda.synchronize()
    assert same(frame.cpu().numpy(), whole)


# 7 ------------------------------------------------------------- accumulator --
# tol 0.1 with the floor 0.01 on the oracle's antialiased frames: the closest
# stop decision of either rule is 5.9e-3 relative from tol (counts, list
# lengths, margin)
RUNS = {(4, 16, 4): (0.1, {4: 34, 8: 7, 12: 8, 16: 95}, [144, 110, 103, 95], 5.897e-3),
        (3, 17, 5): (0.1, {3: 46, 8: 7, 13: 11, 17: 80}, [144, 98, 91, 80], 5.897e-3)}


@pytest.mark.parametrize("rule", list(RUNS), ids=lambda r: "min%d_max%d_step%d" % r)
def test_runs_equal_the_single_kernel_and_the_oracle_simulation(mesh, ref12, rule):
    tol, hist, lengths, margin = RUNS[rule]
    mn, mx, st = rule
    sim = simulate(ref12[:mx], tol, FLOOR, mn, mx, st)
    print(f"rule {rule} tol {tol}: counts {histogram(sim['n'])}, lists {[a for a, _ in sim['passes']]}, "
          f"margin {sim['margin']:.3e}")
    assert sim["margin"] >= 1e-6      # sums that differ by 1e-12 cannot flip a count
    assert 0.95 * margin <= sim["margin"] <= 1.05 * margin
    assert histogram(sim["n"]) == hist and [a for a, _ in sim["passes"]] == lengths
    d, passes = run(mesh, MESH, rule, tol)
    mk, passes_mk = run(mesh, MESH, rule, tol, megakernel=True)
    assert same_bits(d, mk) and passes == passes_mk
    assert np.array_equal(d["n"], sim["n"]) and passes == sim["passes"]
    dS, dQ = float(np.abs(d["S"] - sim["S"]).max()), float(np.abs(d["Q"] - sim["Q"]).max())
    print(f"|S - oracle| = {dS:.3e}, |Q - oracle| = {dQ:.3e}")
    assert dS <= TOL and dQ <= TOL


def test_mixed_n_and_k_in_one_pass(mesh):
    """After the (3, 17, 5) run the pixels hold n = 3, 8, 13, 17; one pass of
    rule (min 10, max 20, step 6, tol 0) adds k = 6, 2, 6, 3: two slots per
    entry with unequal shares, sample0 = n[e] + c differing between entries."""
    W, H, B, seed = MESH
    out = {}
    for mkern in (False, True):
        with Accumulator(mesh, W, H) as acc:
            run_passes(acc, mesh.params(W, H, 17, B, seed, megakernel=mkern, aa=True),
                       make_adapt(0.1, 17, 3, 5, FLOOR))
            n0 = acc.read(n=True)["n"]
            a2 = make_adapt(0.0, 20, 10, 6, FLOOR)
            assert acc.select(a2)[0] == W * H
            acc.render(mesh.params(W, H, 20, B, seed, megakernel=mkern, aa=True), a2)
            out[mkern] = acc.read(S=True, Q=True, n=True)
    assert histogram(n0) == {3: 46, 8: 7, 13: 11, 17: 80}
    k = k_numpy(n0, 10, 20, 6)
    assert histogram(k) == {2: 7, 3: 80, 6: 57}
    assert np.array_equal(out[False]["n"], n0 + k)
    assert same_bits(out[False], out[True])


def test_bands_and_resumed_runs_equal_one_accumulator(mesh, mesh_golden, tmp_path):
    kw = dict(max_spp=16, bounces=3, seed=5, tol=0.1, min_spp=4, step_spp=4, floor=FLOOR,
              lanes_per_pixel=4, aa=True, moments=True)
    one = render_adaptive(mesh, 12, 12, **kw)
    m = MultiRenderer(mesh_golden[0], [0, 0])
    try:
        two = render_adaptive_multi(m.renderers, 12, 12, **kw)
    finally:
        m.close()
    for k in ("S", "Q", "counts", "err"):
        assert same(getattr(one, k), getattr(two, k)), k
    ck = str(tmp_path / "aa_accum.npz")
    assert render_adaptive(mesh, 12, 12, checkpoint=ck, max_passes=2, **kw) is None
    res = render_adaptive(mesh, 12, 12, checkpoint=ck, **kw)
    for k in ("S", "Q", "counts", "err"):
        assert same(getattr(one, k), getattr(res, k)), k
    assert res.passes == one.passes and len(one.passes) == 4


# 8 ------------------------------------------------------------ larger trees --
def test_k5_generator_scene(k5mini_golden):
    with Renderer(k5mini_golden[0]) as r:
        fb, mk = both(r, 10, 6, 4, 3, 9)
        assert same(fb, mk) and fb.any()
        _, d = one_pass(r, (10, 6, 3, 9), 4, PT_FLAG_AA, stats=False)
        _, m = one_pass(r, (10, 6, 3, 9), 4, PT_FLAG_AA | PT_FLAG_MEGAKERNEL, stats=False)
        assert same_bits(d, m)


def test_sliver_scene_through_the_spilled_stacks(tmp_path):
    """The per-sample primary rays go through the walks' spilled stacks: at
    least one closest query per sample of the pass."""
    frame = (16, 16, 4, 9)
    with Renderer(sliver_scene(tmp_path)) as r:
        fb, mk = both(r, 16, 16, 2, 4, 9)
        st, d = one_pass(r, frame, 2, PT_FLAG_AA | PT_FLAG_WALK_COUNT)
        _, m = one_pass(r, frame, 2, PT_FLAG_AA | PT_FLAG_MEGAKERNEL, stats=False)
    assert same(fb, mk) and fb.any() and same_bits(d, m)
    print(f"sliver: closest queries {st['closest_queries']}, node visits {st['closest_node_visits']}")
    assert st["closest_queries"] >= 16 * 16 * 2
    assert st["shadow_queries"] > 0 and st["closest_node_visits"] > 0


# 9 ---------------------------------------------------------- shared buffers --
def test_interleaved_launches_share_the_buffers(mesh):
    W, H, B, seed = MESH
    aa = lambda: mesh.render(W, H, 5, B, seed, out_f64=True, aa=True)
    centre = lambda: mesh.render(9, 4, 6, B, seed, out_f64=True)
    lst = lambda: one_pass(mesh, (7, 5, 3, 11), 4, PT_FLAG_AA, stats=False)[1]
    alone = aa(), centre(), lst()
    got = aa(), centre(), lst(), aa(), lst(), centre(), aa()
    assert same(got[0], alone[0]) and same(got[3], alone[0]) and same(got[6], alone[0])
    assert same(got[1], alone[1]) and same(got[5], alone[1])
    assert same_bits(got[2], alone[2]) and same_bits(got[4], alone[2])
    assert not same(alone[0], mesh.render(W, H, 5, B, seed, out_f64=True))


# 10 ------------------------------------------------------------- validation --
def test_validation_and_the_handle_afterwards(mesh):
    W, H, B, seed = MESH
    before = mesh.render(W, H, 4, B, seed, out_f64=True)
    p = mesh.params(W, H, 4, B, seed, aa=True)
    with pytest.raises(_native.NativeError, match=REFUSED):
        mesh.render_params(with_flags(p, PT_FLAG_COUNT), stats=True)
    with pytest.raises(_native.NativeError, match=REFUSED):
        mesh.render_params(with_flags(p, PT_FLAG_COUNT | PT_FLAG_KERNEL_TIMES), stats=True)
    mesh.render_params(with_flags(p, PT_FLAG_WALK_COUNT), stats=True)      # the handle is usable
    assert same(mesh.render(W, H, 4, B, seed, out_f64=True), before)


# 11 ----------------------------------------------------------- command line --
def test_command_line_flag(mesh, tmp_path, capsys):
    sys.path.insert(0, GOLDEN)
    import mesh_scene as ms
    from pathtracerpython_amd import main as cli
    sdl = ms.write_mesh_scene(str(tmp_path), os.path.dirname(CORNELL))
    base = [sdl, "-r", "4", "-b", "2", "--size", "12", "12", "--seed", "5", "--aa"]
    want = mesh.render(12, 12, 4, 2, 5, out_f64=True, aa=True)
    assert same(np.asarray(cli.main(base), dtype=np.float64), want)
    res = render_adaptive(mesh, 12, 12, 4, 2, 5, tol=0.05, min_spp=2, step_spp=2, aa=True, denoise=True)
    noise = ["--noise", "0.05", "--min-spp", "2", "--step-spp", "2", "--denoise"]
    assert same(cli.main(base + noise), res.denoised)
    capsys.readouterr()
