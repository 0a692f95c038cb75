"""The material scenes (tests/material_scenes.py) on the GPU: exponents that are
no small integer, kd = 0, ks = 0.  They reach the out-of-line f64 pow behind
pow_ref (pt_core.h) from divergent lanes of k_render, its COUNT and FORCE_F64
instantiations, k_render_aa, k_render_list, the BVH single kernel and the
wavefront shade kernel, and they produce the NaN samples that
np.float64 ** float gives the reference for a negative base and a fractional
exponent.  Every comparison is material_scenes.compare: NaN at the oracle's
elements and nowhere else, the rest to 1e-12 (f32 output: 1e-6).  The frames
are the ones tests/test_materials_host.py proves on the host build first: the
oracle equals the reference's own renders there, and 12 .. 21 % of the
sample-pixels of frac, neg and the mesh scene are NaN."""
import glob
import os

import numpy as np
import pytest

import aa_ref
import material_scenes as ms
from adaptive_sim import histogram, simulate
from conftest import GOLDEN
from material_scenes import compare, same_bits
from oracle import oracle
from pathtracerpython_amd.pack import pack_scene
from pathtracerpython_amd.render import Renderer, from_list_order, to_list_order

pytestmark = pytest.mark.gpu

TOL = 1e-12
TOL32 = 1e-6
RR_MODES = [(False, 3), (True, 1), (True, 3)]
RULE = (4, 16, 4)            # min_spp, max_spp, step_spp
ADAPT_TOL, FLOOR = 0.05, 0.01
LANES_FRAME = (16, 16, 64, 3, 9)     # W, H, spp, bounces, seed


@pytest.fixture(scope="module")
def R(tmp_path_factory):
    """{case: Renderer}"""
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    out = {}
    try:
        for case in ms.SCENES:
            sc = ms.material_scene(tmp_path_factory.mktemp("mat_" + case), case)
            out[case] = Renderer(sc, packed=pack_scene(sc))
        yield out
    finally:
        for r in out.values():
            r.close()


# 1 ------------------------------------------------------------------ parity --
@pytest.mark.parametrize("rr,rr_depth", RR_MODES, ids=["norr", "rr1", "rr3"])
@pytest.mark.parametrize("case", ms.SCENES)
def test_per_sample_frames_equal_the_oracle(R, case, rr, rr_depth):
    """Every per-sample frame: f64 output to 1e-12 and f32 output to 1e-6 with
    the oracle's NaN positions, the COUNT instantiation's frame and counters,
    and the other kernel of the scene bit for bit — forced f64 for the uniform
    scenes (k_render), the single kernel for the mesh scene (the wavefront
    kernels by default)."""
    r = R[case]
    ref, ostats = ms.oracle_frames(r.packed, case, rr, rr_depth)
    W, H, B, seed = ms.FRAME
    other = dict(megakernel=True) if case == "mesh" else dict(force_f64=True)
    worst = worst32 = 0.0
    for s in range(len(ref)):
        kw = dict(rr=rr, rr_depth=rr_depth, sample_begin=s)
        what = f"{case} sample {s} rr {rr} depth {rr_depth}"
        fb = r.render(W, H, 1, B, seed, out_f64=True, **kw)
        worst = max(worst, compare(fb, ref[s], TOL, what)[1])
        f32 = r.render(W, H, 1, B, seed, **kw)
        assert f32.dtype == np.float32
        worst32 = max(worst32, compare(f32, ref[s], TOL32, what + " f32")[1])
        assert same_bits(r.render(W, H, 1, B, seed, out_f64=True, **other, **kw), fb), what
        cfb, st = r.render(W, H, 1, B, seed, out_f64=True, stats=True, **kw)
        compare(cfb, ref[s], TOL, what + " count")
        for k in ms.COUNTERS:
            assert st[k] == ostats[s][k], (what, k)
        if case not in ms.NAN_SCENES:
            assert np.isfinite(fb).all() and np.isfinite(f32).all()
    print(f"{case} rr {rr} depth {rr_depth}: f64 {worst:.3e}, f32 {worst32:.3e}, "
          f"NaN sample-pixels {ms.nan_share(ref):.3f}")


@pytest.mark.parametrize("name", sorted(os.path.basename(f)
                                        for f in glob.glob(os.path.join(GOLDEN, "mat_*.npz"))))
def test_frames_equal_the_reference_renders(R, name):
    """The reference's own renders (gen_golden.py materials), NaN pixels
    included."""
    g = np.load(os.path.join(GOLDEN, name))
    case = name.split("_")[1]
    W, H, spp, B, seed = (int(g[k]) for k in ("width", "height", "spp", "bounces", "seed"))
    fb = R[case].render(W, H, spp, B, seed, out_f64=True)
    nan, worst = compare(to_list_order(fb), g["colors"], TOL, name)
    print(f"{name}: {nan // 3} NaN pixels of {W * H}, {worst:.3e}")
    compare(to_list_order(R[case].render(W, H, spp, B, seed)), g["colors"], TOL32, name + " f32")
    assert (nan > 0) == (case in ms.NAN_SCENES)


# 2 ------------------------------------------------------------------- lanes --
@pytest.fixture(scope="module")
def lanes_ref(R):
    W, H, spp, B, seed = LANES_FRAME
    ref, _ = oracle.render(R["frac"].packed, W, H, spp, B, seed)
    ref = from_list_order(ref, W, H)
    nan_px = np.isnan(ref).any(axis=-1)
    assert 40 <= nan_px.sum() <= W * H - 40      # (seed 9: 158 of 256)
    return ref


@pytest.mark.parametrize("lanes", [0, 1, 64])
def test_lane_sums_carry_a_nan(R, lanes_ref, lanes):
    """64 samples of a pixel over 1, 64 or the library's choice of lanes: one
    NaN sample makes the butterfly sum NaN in every lane count, and no other
    pixel's."""
    W, H, spp, B, seed = LANES_FRAME
    fb = R["frac"].render(W, H, spp, B, seed, out_f64=True, lanes_per_pixel=lanes)
    compare(fb, lanes_ref, TOL, f"lanes {lanes}")
    compare(R["frac"].render(W, H, spp, B, seed, lanes_per_pixel=lanes), lanes_ref, TOL32,
            f"lanes {lanes} f32")


# 3 --------------------------------------------------- sample splits, bands --
def test_sample_chunks_and_row_bands_reproduce_the_frame(R):
    from pathtracerpython_amd.distributed import assemble, max_band_rows
    r = R["frac"]
    W, H, B, seed = ms.FRAME
    whole = r.render(W, H, 8, B, seed, out_f64=True, lanes_per_pixel=4)
    assert 0 < np.isnan(whole).any(axis=-1).sum() < W * H
    a = r.render(W, H, 4, B, seed, out_f64=True, lanes_per_pixel=4)
    b = r.render(W, H, 4, B, seed, out_f64=True, lanes_per_pixel=4, sample_begin=4)
    compare((a * 4 + b * 4) / 8, whole, 1e-14, "two sample chunks")
    tiles = []
    for ph in range(2):
        t = r.render(W, H, 8, B, seed, out_f64=True, lanes_per_pixel=4, row_step=2, row_phase=ph)
        pad = np.zeros((max_band_rows(H, 2), W, 3))
        pad[:t.shape[0]] = t
        tiles.append(pad)
    assert same_bits(assemble(tiles, H), whole)
    ref, _ = oracle.render(r.packed, W, H, 8, B, seed)
    compare(to_list_order(whole), ref, TOL, "8 spp")


# 4 ---------------------------------------------------------------------- AA --
def test_antialiased_frame_equals_the_shifted_window_oracle(R):
    """k_render_aa has its own instantiation of the bounce loop."""
    r = R["frac"]
    W, H, spp, B, seed = 12, 12, 4, 4, 9
    c = aa_ref.to_image(aa_ref.aa_samples(r.scene, W, H, B, seed, spp), W, H)
    ref = c.sum(axis=0) / spp
    nan_px = np.isnan(ref).any(axis=-1)
    assert 10 <= nan_px.sum() <= W * H - 10
    fb = r.render(W, H, spp, B, seed, out_f64=True, aa=True)
    compare(fb, ref, TOL, "aa")
    assert same_bits(r.render(W, H, spp, B, seed, out_f64=True, aa=True, force_f64=True), fb)
    compare(r.render(W, H, spp, B, seed, aa=True), ref, TOL32, "aa f32")


# 5 ---------------------------------------------------------------- adaptive --
@pytest.mark.parametrize("case,megakernel", [("frac", False), ("mesh", False), ("mesh", True)],
                         ids=["frac", "mesh-wavefront", "mesh-megakernel"])
def test_adaptive_run_equals_the_simulation(R, case, megakernel):
    """render_adaptive (k_render_list; the wavefront list form and the single
    kernel for the mesh scene) against adaptive_sim on the oracle's frames:
    the count map pixel for pixel, S and Q, err with NaN at the same pixels.
    A pixel with a NaN sum leaves the list once n >= min_spp (err > tol is
    false for NaN), so the run ends within (max - min) / step + 1 passes."""
    r = R[case]
    W, H, B, seed = ms.FRAME
    mn, mx, st = RULE
    c, _ = ms.oracle_frames(r.packed, case, n_samples=mx)
    sim = simulate(c, ADAPT_TOL, FLOOR, mn, mx, st)
    print(f"{case}: counts {histogram(sim['n'])}, passes {sim['passes']}, margin {sim['margin']:.3e}")
    assert sim["margin"] >= 1e-6            # sums 1e-12 apart flip no stop decision
    nan_px = np.isnan(sim["S"]).any(axis=-1)
    assert 40 <= nan_px.sum() <= W * H - 40
    res = r.render_adaptive(W, H, mx, B, seed, tol=ADAPT_TOL, min_spp=mn, step_spp=st, floor=FLOOR,
                            megakernel=megakernel, moments=True)
    assert np.array_equal(res.counts, sim["n"])
    assert res.passes == sim["passes"] and len(res.passes) <= (mx - mn) // st + 1
    compare(res.S, sim["S"], TOL, "S")
    compare(res.Q, sim["Q"], TOL, "Q")
    assert np.array_equal(np.isnan(res.err), np.isnan(sim["err"]))
    assert np.array_equal(np.isnan(res.err), nan_px)
    compare(res.fb, sim["mean"], TOL, "mean")


# 6 -------------------------------------------------------------- edge cases --
def test_zero_throughput_ends_the_colour(R):
    """zero: a path whose first hit is cube2 (kd = ks = 0) adds nothing
    afterwards: its pixels after 5 bounces hold what 1 bounce gives them, and
    that is the oracle's."""
    r = R["zero"]
    W, H, B, seed = ms.FRAME
    first = ms.first_hit_objects(r.packed, W, H) == ms.CUBE2
    assert 10 <= first.sum() < W * H // 2
    deep = r.render(W, H, 2, B, seed, out_f64=True)
    one = r.render(W, H, 2, 1, seed, out_f64=True)
    assert np.isfinite(deep).all()
    assert np.array_equal(deep[first], one[first])
    assert not np.array_equal(deep[~first], one[~first])
    ref, _ = oracle.render(r.packed, W, H, 2, B, seed)
    ref1, _ = oracle.render(r.packed, W, H, 2, 1, seed)
    compare(to_list_order(deep), ref, TOL, "zero, 5 bounces")
    compare(to_list_order(one), ref1, TOL, "zero, 1 bounce")
