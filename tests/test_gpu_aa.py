"""Antialiasing on the GPU (PT_FLAG_AA, include/pt_capi.h; pt_aa.hip
k_render_aa / k_render_list_aa): the frames against the oracle on shifted
screen windows (tests/aa_ref.py), sample ranges, bands, the forced-f64
self-check, BVH scenes through the single kernel, the accumulator and the
argument checks.  Host-side cases: tests/test_aa_host.py."""
import numpy as np
import pytest

import aa_ref
from adaptive_sim import histogram, simulate
from conftest import quad_scene
from pathtracerpython_amd import _native
from pathtracerpython_amd._abi import (PT_FLAG_AA, PT_FLAG_COUNT, PT_FLAG_KERNEL_TIMES,
                                       PT_FLAG_WALK_COUNT, make_adapt, with_flags)
from pathtracerpython_amd.adaptive import (Accumulator, render_adaptive, render_adaptive_multi,
                                           run_passes)
from pathtracerpython_amd.pack import pack_scene
from pathtracerpython_amd.progressive import render_progressive
from pathtracerpython_amd.render import MultiRenderer, Renderer

pytestmark = pytest.mark.gpu

TOL = 1e-12
FLOOR = 1e-3     # tests/test_aa_host.py: the stop decisions' margin with it is 1.6e-3


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else a.dtype)


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


@pytest.fixture(scope="module")
def R(cornell):
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    with Renderer(cornell) as r:
        yield r


@pytest.fixture(scope="module")
def ref12(cornell):
    """Cornell 12x12, 8 samples, 3 bounces, seed 9, image orientation; every
    branch of the restart loop is in it."""
    c = aa_ref.aa_samples(cornell, 12, 12, 3, 9, 8)
    me, ml, ae = aa_ref.coverage(c, pack_scene(cornell).light_rgb)
    assert me >= 1 and ml >= 1 and ae >= 1
    return aa_ref.to_image(c, 12, 12)


@pytest.fixture(scope="module")
def ref75(cornell):
    return aa_ref.to_image(aa_ref.aa_samples(cornell, 7, 5, 3, 9, 8), 7, 5)


@pytest.fixture(scope="module")
def ref16(cornell):
    return aa_ref.to_image(aa_ref.aa_samples(cornell, 16, 16, 3, 9, 17), 16, 16)


def mean_err(fb, ref, spp):
    return float(np.abs(fb - ref[:spp].sum(axis=0) / spp).max())


# 1 ----------------------------------------------------------- oracle parity --
def test_frame_matches_the_oracle(R, ref12):
    fb = R.render(12, 12, 8, 3, 9, out_f64=True, aa=True)
    e = mean_err(fb, ref12, 8)
    print(f"12x12x8 aa vs oracle: {e:.3e}")
    assert e <= TOL
    f32 = R.render(12, 12, 8, 3, 9, aa=True)
    assert f32.dtype == np.float32 and mean_err(f32.astype(np.float64), ref12, 8) <= 1e-6
    # antialiasing is on: the frame is not the centre-ray one
    assert np.abs(fb - R.render(12, 12, 8, 3, 9, out_f64=True)).max() > 1e-3


@pytest.mark.parametrize("spp,lanes", [(5, 4), (7, 2), (8, 1)])
def test_uneven_lanes_match_the_oracle(R, ref75, spp, lanes):
    fb = R.render(7, 5, spp, 3, 9, out_f64=True, aa=True, lanes_per_pixel=lanes)
    assert fb.shape == (5, 7, 3) and mean_err(fb, ref75, spp) <= TOL


@pytest.mark.parametrize("lanes", [16, 64])
def test_wide_pixels_match_the_oracle(R, cornell, lanes):
    """16 lanes was primary_shared's threshold; 64 is one sample per lane."""
    ref = aa_ref.to_image(aa_ref.aa_samples(cornell, 6, 6, 2, 9, 64), 6, 6)
    fb = R.render(6, 6, 64, 2, 9, out_f64=True, aa=True, lanes_per_pixel=lanes)
    assert mean_err(fb, ref, 64) <= TOL


def test_russian_roulette_tiny_frames_and_no_bounces(R, cornell):
    from pathtracerpython_amd._abi import PT_FLAG_RR
    ref = aa_ref.to_image(aa_ref.aa_samples(cornell, 12, 12, 4, 9, 8, flags=PT_FLAG_RR), 12, 12)
    fb = R.render(12, 12, 8, 4, 9, rr=True, out_f64=True, aa=True)
    assert mean_err(fb, ref, 8) <= TOL
    for W, H in ((1, 1), (3, 1)):
        ref = aa_ref.to_image(aa_ref.aa_samples(cornell, W, H, 3, 9, 4), W, H)
        fb = R.render(W, H, 4, 3, 9, out_f64=True, aa=True)
        assert fb.shape == (H, W, 3) and mean_err(fb, ref, 4) <= TOL
    assert not R.render(12, 12, 8, 0, 9, out_f64=True, aa=True).any()


# 2 ----------------------------------------------------------- sample ranges --
def test_sample_ranges_and_chunks(R, ref12, tmp_path):
    fb = R.render(12, 12, 3, 3, 9, out_f64=True, aa=True, sample_begin=5)
    assert np.abs(fb - ref12[5:8].sum(axis=0) / 3).max() <= TOL
    one = R.render(12, 12, 8, 3, 9, out_f64=True, aa=True)
    two = render_progressive(R, 12, 12, 8, 3, 9, chunk_spp=4, aa=True)
    assert np.abs(two - one).max() <= 1e-14
    ck = str(tmp_path / "aa.npz")
    assert render_progressive(R, 12, 12, 8, 3, 9, chunk_spp=4, checkpoint=ck, max_chunks=1,
                              aa=True) is None
    with pytest.raises(ValueError, match="another render"):   # resuming an AA file without aa
        render_progressive(R, 12, 12, 8, 3, 9, chunk_spp=4, checkpoint=ck)
    resumed = render_progressive(R, 12, 12, 8, 3, 9, chunk_spp=4, checkpoint=ck, aa=True)
    assert same(resumed, two)


# 3 ------------------------------------------------------------------- bands --
def test_bands_equal_the_whole_frame_bit_for_bit(R):
    import torch
    W, H, spp = 7, 5, 8
    whole = R.render(W, H, spp, 3, 9, out_f64=True, aa=True, lanes_per_pixel=4)
    s = torch.cuda.current_stream().cuda_stream
    # interleaved rows, both phases
    frame = torch.full((H, W, 3), float("nan"), dtype=torch.float64, device="cuda")
    for phase in range(2):
        iy_top = max(range(phase, H, 2))
        p = R.params(W, H, spp, 3, 9, out_f64=True, aa=True, lanes_per_pixel=4, row_step=2,
                     row_phase=phase, out_row_stride=2 * W * 3)
        R.render_device(p, frame[H - 1 - iy_top].data_ptr(), s)
    torch.cuda.synchronize()
    assert same(frame.cpu().numpy(), whole)
    # a contiguous split: rows 0..1 and 2..4
    frame = torch.full((H, W, 3), float("nan"), dtype=torch.float64, device="cuda")
    for rb, re in ((0, 2), (2, 5)):
        p = R.params(W, H, spp, 3, 9, out_f64=True, aa=True, lanes_per_pixel=4, row_begin=rb,
                     row_end=re, out_row_stride=W * 3)
        R.render_device(p, frame[H - re].data_ptr(), s)
    torch.cuda.synchronize()
    assert same(frame.cpu().numpy(), whole)


# 4 -------------------------------------------------------------- self-check --
def test_forced_f64_equals_the_hybrid_filter(R, tmp_path):
    a = R.render(32, 32, 4, 4, 9, out_f64=True, aa=True)
    assert same(a, R.render(32, 32, 4, 4, 9, out_f64=True, aa=True, force_f64=True))
    with Renderer(quad_scene(tmp_path, 3)) as q:
        b = q.render(12, 12, 3, 4, 3, out_f64=True, aa=True)
        assert b.any() and same(b, q.render(12, 12, 3, 4, 3, out_f64=True, aa=True, force_f64=True))


# 5 --------------------------------------------------------------------- BVH --
def test_bvh_scene_through_the_single_kernel(mesh_golden):
    """A launch that went through the wavefront kernels would hold the
    centre-ray frame (they have no per-sample primary query): the antialiased
    frame within 1e-12 of the oracle, and the kernel time of the handle set,
    say that the single kernel ran."""
    sc, _ = mesh_golden
    ref = aa_ref.to_image(aa_ref.aa_samples(sc, 12, 12, 3, 5, 2), 12, 12)
    with Renderer(sc) as r:
        fb = r.render(12, 12, 2, 3, 5, out_f64=True, aa=True)
        assert r.last_kernel_ms() > 0.0
        assert mean_err(fb, ref, 2) <= TOL
        assert same(fb, r.render(12, 12, 2, 3, 5, out_f64=True, aa=True, megakernel=True))
        centre = r.render(12, 12, 2, 3, 5, out_f64=True)   # the wavefront kernels
        assert np.abs(fb - centre).max() > 1e-3
        # the accumulator's pass: the same samples, wavefront or not asked for
        adapt = make_adapt(0.0, 2, 2, 2)
        got = []
        for mk in (False, True):
            with Accumulator(r, 12, 12) as acc:
                run_passes(acc, r.params(12, 12, 2, 3, 5, aa=True, megakernel=mk), adapt)
                got.append(acc.read(S=True, Q=True, n=True))
        assert all(same(got[0][k], got[1][k]) for k in ("S", "Q", "n"))
        assert np.abs(got[0]["S"] - ref.sum(axis=0)).max() <= TOL
        assert np.abs(got[0]["Q"] - (ref ** 2).sum(axis=0)).max() <= TOL


# 6 ------------------------------------------------------------- accumulator --
RULES = [((4, 16, 4), {4: 46, 8: 31, 12: 13, 16: 166}), ((3, 17, 5), {3: 53, 8: 31, 13: 13, 17: 159})]


@pytest.mark.parametrize("rule,hist", RULES)
def test_adaptive_counts_equal_the_simulation(R, ref16, rule, hist):
    mn, mx, st = rule
    sim = simulate(ref16[:mx], 0.05, FLOOR, mn, mx, st)
    assert sim["margin"] >= 1e-6 and histogram(sim["n"]) == hist
    res = render_adaptive(R, 16, 16, mx, 3, 9, tol=0.05, min_spp=mn, step_spp=st, floor=FLOOR,
                          aa=True, moments=True)
    assert np.array_equal(res.counts, sim["n"]) and res.passes == sim["passes"]
    assert np.abs(res.S - sim["S"]).max() <= TOL and np.abs(res.Q - sim["Q"]).max() <= TOL


def test_bands_and_resumed_runs_equal_one_accumulator(R, cornell, tmp_path):
    kw = dict(max_spp=16, bounces=3, seed=9, tol=0.05, min_spp=4, step_spp=4, floor=FLOOR,
              lanes_per_pixel=4, aa=True, moments=True)
    one = render_adaptive(R, 16, 16, **kw)
    m = MultiRenderer(cornell, [0, 0])
    try:
        two = render_adaptive_multi(m.renderers, 16, 16, **kw)
    finally:
        m.close()
    for k in ("S", "Q", "counts", "err"):
        assert same(getattr(one, k), getattr(two, k)), k
    ck = str(tmp_path / "aa_accum.npz")
    assert render_adaptive(R, 16, 16, checkpoint=ck, max_passes=2, **kw) is None
    with pytest.raises(ValueError, match="another render"):
        render_adaptive(R, 16, 16, checkpoint=ck, **{**kw, "aa": False})
    res = render_adaptive(R, 16, 16, checkpoint=ck, **kw)
    for k in ("S", "Q", "counts", "err"):
        assert same(getattr(one, k), getattr(res, k)), k
    assert res.passes == one.passes


def test_accumulator_refuses_mixed_passes(R):
    adapt = make_adapt(0.0, 4, 4, 2)      # every pixel: two passes of two samples
    p = R.params(8, 8, 4, 2, 9)
    with Accumulator(R, 8, 8) as acc:
        acc.render(with_flags(p, PT_FLAG_AA), adapt)
        with pytest.raises(_native.NativeError, match=r"\(-1\): .*PT_FLAG_AA"):
            acc.render(p, adapt)
        acc.render(with_flags(p, PT_FLAG_AA), adapt)       # the handle is still usable
        assert (acc.read(n=True)["n"] == 4).all()
        acc.reset()
        acc.render(p, adapt)                                # after a reset either value
        with pytest.raises(_native.NativeError, match=r"\(-1\): .*PT_FLAG_AA"):
            acc.render(with_flags(p, PT_FLAG_AA), adapt)
        d = acc.read(S=True, Q=True, n=True)
        acc.write(d["S"], d["Q"], d["n"])                   # the caller vouches for the state
        acc.render(with_flags(p, PT_FLAG_AA), adapt)
        assert (acc.read(n=True)["n"] == 4).all()


def test_denoise_and_features_keep_the_centre_ray(R):
    adapt = make_adapt(0.0, 4, 4, 4)
    with Accumulator(R, 16, 16) as a, Accumulator(R, 16, 16) as b:
        run_passes(a, R.params(16, 16, 4, 3, 9, aa=True), adapt)
        run_passes(b, R.params(16, 16, 4, 3, 9), adapt)
        before = a.read(S=True, Q=True, n=True)
        den, var = a.denoise()
        after = a.read(S=True, Q=True, n=True)
        assert all(same(before[k], after[k]) for k in ("S", "Q", "n"))
        assert np.isfinite(den).all() and np.isfinite(var).all()
        fa, fb = a.features(), b.features()
        assert all(same(fa[k], fb[k]) for k in ("tri", "obj", "N", "P"))
        assert not same(before["S"], b.read(S=True)["S"])


# 7 -------------------------------------------------------------- validation --
def test_validation_and_the_handle_afterwards(R):
    before = R.render(12, 12, 4, 3, 9, out_f64=True)
    p = R.params(12, 12, 4, 3, 9, aa=True)
    for flag in (PT_FLAG_COUNT, PT_FLAG_WALK_COUNT, PT_FLAG_KERNEL_TIMES):
        with pytest.raises(_native.NativeError, match=r"\(-1\): .*PT_FLAG_AA"):
            R.render_params(with_flags(p, flag))
    for bit in (1 << 7, 1 << 20):
        with pytest.raises(_native.NativeError, match=r"\(-1\): .*flag"):
            R.render_params(with_flags(p, bit))
    with Accumulator(R, 12, 12) as acc:
        for flag in (PT_FLAG_WALK_COUNT, PT_FLAG_KERNEL_TIMES):
            with pytest.raises(_native.NativeError, match=r"\(-1\): .*PT_FLAG_AA"):
                acc.render(with_flags(p, flag), make_adapt(0.0, 4, 4, 4))
    R.render(12, 12, 4, 3, 9, out_f64=True, aa=True)
    # a render without the flag right after an antialiased one on the handle
    assert same(R.render(12, 12, 4, 3, 9, out_f64=True), before)


# 8 --------------------------------------------------------------------- CLI --
def test_command_line_flag(R, tmp_path, capsys):
    """--aa alone, with --chunk-spp / --checkpoint, with --noise --denoise and
    with --local-devices: the frames the library calls give."""
    from conftest import CORNELL
    from pathtracerpython_amd import main as cli
    base = [CORNELL, "-r", "4", "-b", "2", "--size", "12", "12", "--seed", "9", "--aa"]
    want = R.render(12, 12, 4, 2, 9, out_f64=True, aa=True)
    assert same(np.asarray(cli.main(base), dtype=np.float64), want)
    ck = str(tmp_path / "cli.npz")
    fb = cli.main(base + ["--chunk-spp", "2", "--checkpoint", ck])
    assert np.abs(fb - want).max() <= 1e-14
    with pytest.raises(ValueError, match="another render"):   # the file is an antialiased run's
        cli.main(base[:-1] + ["--chunk-spp", "2", "--checkpoint", ck])
    res = render_adaptive(R, 12, 12, 4, 2, 9, tol=0.05, min_spp=2, step_spp=2, aa=True, denoise=True)
    noise = ["--noise", "0.05", "--min-spp", "2", "--step-spp", "2", "--denoise"]
    assert same(cli.main(base + noise), res.denoised)
    assert np.abs(cli.main(base + noise + ["--local-devices", "1"]) - res.denoised).max() <= 1e-12
    assert same(np.asarray(cli.main(base + ["--local-devices", "1"]), dtype=np.float64), want)
    capsys.readouterr()
