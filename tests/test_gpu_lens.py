"""The thin-lens camera on the GPU (PT_FLAG_LENS, include/pt_capi.h; pt_lens.hip
k_render_lens / k_render_list_lens): the frames against the oracle on shifted
eyes and screen windows (tests/lens_ref.py), lane counts, sample ranges, bands,
the forced-f64 self-check, Russian roulette, the accumulator, BVH scenes
through the single kernel, the R = 0 equalities, MultiRenderer, the argument
checks and the command line.  Every test that renders with the flag needs the
flag and pt_scene_create_lens.  Host-side cases: tests/test_lens_host.py."""
import numpy as np
import pytest

import lens_ref
from adaptive_sim import histogram, simulate
from pathtracerpython_amd import _native
from pathtracerpython_amd._abi import (PT_FLAG_COUNT, PT_FLAG_KERNEL_TIMES, PT_FLAG_LENS, PT_FLAG_RR,
                                       PT_FLAG_WALK_COUNT, make_adapt, with_flags)
from pathtracerpython_amd.adaptive import Accumulator, render_adaptive, run_passes
from pathtracerpython_amd.pack import pack_scene
from pathtracerpython_amd.progressive import render_progressive
from pathtracerpython_amd.render import MultiRenderer, Renderer

pytestmark = pytest.mark.gpu

TOL = 1e-12
FLOOR = 1e-3     # tests/test_lens_host.py: the stop decisions' margin with it is 4e-3
A, B = lens_ref.CASE_A, lens_ref.CASE_B


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else a.dtype)


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def gpu():
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"


@pytest.fixture(scope="module")
def RA(cornell):
    gpu()
    with Renderer(cornell, lens=(A["R"], A["zf"])) as r:
        yield r


@pytest.fixture(scope="module")
def RB(cornell):
    gpu()
    with Renderer(cornell, lens=(B["R"], B["zf"])) as r:
        yield r


@pytest.fixture(scope="module")
def plain(cornell):
    gpu()
    with Renderer(cornell) as r:
        yield r


def reference(scene, case, want_light):
    c = lens_ref.lens_samples(scene, 12, 12, 3, 9, 8, **case)
    me, ml, ae = lens_ref.coverage(c, pack_scene(scene).light_rgb)
    assert me >= 1 and ae >= 1 and (ml >= 1 or not want_light)
    return lens_ref.to_image(c, 12, 12)


@pytest.fixture(scope="module")
def refA(cornell):
    return reference(cornell, A, True)


@pytest.fixture(scope="module")
def refB(cornell):
    return reference(cornell, B, False)


def mean_err(fb, ref, spp):
    return float(np.abs(fb - ref[:spp].sum(axis=0) / spp).max())


# 1 ----------------------------------------------------------- oracle parity --
def test_case_a_matches_the_oracle(RA, refA):
    fb = RA.render(12, 12, 8, 3, 9, out_f64=True, aa=True)
    e = mean_err(fb, refA, 8)
    print(f"A 12x12x8 vs oracle: {e:.3e}")
    assert e <= TOL
    f32 = RA.render(12, 12, 8, 3, 9, aa=True)
    assert f32.dtype == np.float32 and mean_err(f32.astype(np.float64), refA, 8) <= 1e-6
    # the lens is on: neither the antialiased nor the centre-ray pinhole frame
    assert np.abs(fb - RA.render(12, 12, 8, 3, 9, out_f64=True, aa=True, lens=False)).max() > 1e-3


def test_case_b_matches_the_oracle(RB, refB):
    fb = RB.render(12, 12, 8, 3, 9, out_f64=True)
    e = mean_err(fb, refB, 8)
    print(f"B 12x12x8 vs oracle: {e:.3e}")
    assert e <= TOL
    f32 = RB.render(12, 12, 8, 3, 9)
    assert f32.dtype == np.float32 and mean_err(f32.astype(np.float64), refB, 8) <= 1e-6
    assert np.abs(fb - RB.render(12, 12, 8, 3, 9, out_f64=True, lens=False)).max() > 1e-3
    # several samples per lane without PT_FLAG_AA: the restarts inside the bounce loop
    for lanes in (1, 4, 8):
        fl = RB.render(12, 12, 8, 3, 9, out_f64=True, lanes_per_pixel=lanes)
        assert mean_err(fl, refB, 8) <= TOL, lanes
        assert same(fl, RB.render(12, 12, 8, 3, 9, out_f64=True, lanes_per_pixel=lanes, force_f64=True))


# 2 ----------------------------------------- bitwise with fixed lanes per pixel --
@pytest.mark.parametrize("lanes", [1, 4, 8])
def test_lanes_chunks_bands_and_forced_f64(RA, refA, lanes):
    import torch
    kw = dict(out_f64=True, aa=True, lanes_per_pixel=lanes)
    whole = RA.render(12, 12, 8, 3, 9, **kw)
    assert mean_err(whole, refA, 8) <= TOL
    # forced f64: the same frame bit for bit
    assert same(whole, RA.render(12, 12, 8, 3, 9, force_f64=True, **kw))
    # sample_begin chunks 3 + 5 (each with its own lane count <= its samples)
    cl = min(lanes, 2)
    a = RA.render(12, 12, 3, 3, 9, out_f64=True, aa=True, lanes_per_pixel=cl)
    b = RA.render(12, 12, 5, 3, 9, out_f64=True, aa=True, lanes_per_pixel=min(lanes, 4), sample_begin=3)
    assert np.abs(a - refA[:3].sum(axis=0) / 3).max() <= TOL
    assert np.abs(b - refA[3:8].sum(axis=0) / 5).max() <= TOL
    assert same(a, RA.render(12, 12, 3, 3, 9, out_f64=True, aa=True, lanes_per_pixel=cl))
    # row bands: row_step 2, both phases, into one frame
    s = torch.cuda.current_stream().cuda_stream
    frame = torch.full((12, 12, 3), float("nan"), dtype=torch.float64, device="cuda")
    for phase in range(2):
        iy_top = max(range(phase, 12, 2))
        p = RA.params(12, 12, 8, 3, 9, row_step=2, row_phase=phase, out_row_stride=2 * 12 * 3, **kw)
        RA.render_device(p, frame[12 - 1 - iy_top].data_ptr(), s)
    torch.cuda.synchronize()
    assert same(frame.cpu().numpy(), whole)


def test_resumed_progressive_run(RA, refA, tmp_path):
    one = RA.render(12, 12, 8, 3, 9, out_f64=True, aa=True)
    two = render_progressive(RA, 12, 12, 8, 3, 9, chunk_spp=4, aa=True)
    assert np.abs(two - one).max() <= 1e-14
    ck = str(tmp_path / "lens.npz")
    assert render_progressive(RA, 12, 12, 8, 3, 9, chunk_spp=4, checkpoint=ck, max_chunks=1, aa=True) is None
    with pytest.raises(ValueError, match="another render"):   # a lens file resumed as a pinhole run
        render_progressive(RA, 12, 12, 8, 3, 9, chunk_spp=4, checkpoint=ck, aa=True, lens=False)
    assert same(render_progressive(RA, 12, 12, 8, 3, 9, chunk_spp=4, checkpoint=ck, aa=True), two)


# 3 ------------------------------------------------------- Russian roulette --
def test_russian_roulette_at_depth_one(RA, cornell):
    ref = lens_ref.to_image(lens_ref.lens_samples(cornell, 8, 8, 4, 9, 4, flags=PT_FLAG_RR, rr_depth=1, **A), 8, 8)
    fb = RA.render(8, 8, 4, 4, 9, rr=True, rr_depth=1, out_f64=True, aa=True)
    assert mean_err(fb, ref, 4) <= TOL
    assert not RA.render(8, 8, 4, 0, 9, out_f64=True, aa=True).any()      # no bounces


# 4 ------------------------------------------- list kernel and accumulator --
@pytest.mark.parametrize("case", ["A", "B"])
def test_list_kernel_moments_match_the_oracle(RA, RB, refA, refB, case):
    r, ref, aa = (RA, refA, True) if case == "A" else (RB, refB, False)
    adapt = make_adapt(0.0, 8, 8, 4)             # every pixel: two passes of four samples
    with Accumulator(r, 12, 12) as acc:
        run_passes(acc, r.params(12, 12, 8, 3, 9, aa=aa), adapt)
        d = acc.read(S=True, Q=True, n=True)
    assert (d["n"] == 8).all()
    assert np.abs(d["S"] - ref.sum(axis=0)).max() <= TOL
    assert np.abs(d["Q"] - (ref ** 2).sum(axis=0)).max() <= TOL


@pytest.fixture(scope="module")
def ref16(cornell):
    return lens_ref.to_image(lens_ref.lens_samples(cornell, 16, 16, 3, 9, 17, **A), 16, 16)


def test_adaptive_counts_equal_the_simulation(RA, ref16):
    mn, mx, st = 3, 17, 5
    sim = simulate(ref16[:mx], 0.05, FLOOR, mn, mx, st)
    assert sim["margin"] >= 1e-9 and len(histogram(sim["n"])) >= 3
    res = render_adaptive(RA, 16, 16, mx, 3, 9, tol=0.05, min_spp=mn, step_spp=st, floor=FLOOR,
                          aa=True, moments=True)
    assert np.array_equal(res.counts, sim["n"]) and res.passes == sim["passes"]
    assert np.abs(res.S - sim["S"]).max() <= TOL and np.abs(res.Q - sim["Q"]).max() <= TOL


def test_accumulator_refuses_mixed_passes(RA):
    adapt = make_adapt(0.0, 4, 4, 2)      # every pixel: two passes of two samples
    off = RA.params(8, 8, 4, 2, 9, lens=False)
    on = RA.params(8, 8, 4, 2, 9)
    assert on.flags & PT_FLAG_LENS and not off.flags & PT_FLAG_LENS
    with Accumulator(RA, 8, 8) as acc:
        acc.render(on, adapt)
        with pytest.raises(_native.NativeError, match=r"\(-1\): .*PT_FLAG_LENS"):
            acc.render(off, adapt)
        acc.render(on, adapt)                               # the handle is still usable
        assert (acc.read(n=True)["n"] == 4).all()
        acc.reset()
        acc.render(off, adapt)                              # after a reset either value
        with pytest.raises(_native.NativeError, match=r"\(-1\): .*PT_FLAG_LENS"):
            acc.render(on, adapt)


# 5 --------------------------------------------------------------------- BVH --
def test_bvh_scene_through_the_single_kernel(mesh_golden):
    """With the flag a BVH scene takes the single kernel (BVH = true): the
    wavefront kernels have no lens form, and a launch through them would hold
    the pinhole frame."""
    gpu()
    sc, _ = mesh_golden
    ref = lens_ref.to_image(lens_ref.lens_samples(sc, 12, 12, 3, 5, 2, **A), 12, 12)
    with Renderer(sc, lens=(A["R"], A["zf"])) as r:
        fb = r.render(12, 12, 2, 3, 5, out_f64=True, aa=True)
        assert r.last_kernel_ms() > 0.0
        assert mean_err(fb, ref, 2) <= TOL
        assert same(fb, r.render(12, 12, 2, 3, 5, out_f64=True, aa=True, megakernel=True))
        assert same(fb, r.render(12, 12, 2, 3, 5, out_f64=True, aa=True, force_f64=True))
        pin = r.render(12, 12, 2, 3, 5, out_f64=True, aa=True, lens=False)   # the wavefront kernels
        assert np.abs(fb - pin).max() > 1e-3
        # the wavefront kernels' stats are not to be had with the flag
        for flag in (PT_FLAG_WALK_COUNT, PT_FLAG_KERNEL_TIMES):
            with pytest.raises(_native.NativeError, match=r"\(-1\): .*PT_FLAG_LENS"):
                r.render_params(with_flags(r.params(12, 12, 2, 3, 5, aa=True), flag))
        adapt = make_adapt(0.0, 2, 2, 2)
        with Accumulator(r, 12, 12) as acc:
            run_passes(acc, r.params(12, 12, 2, 3, 5, aa=True), adapt)
            d = acc.read(S=True, Q=True, n=True)
        assert np.abs(d["S"] - ref.sum(axis=0)).max() <= TOL
        assert np.abs(d["Q"] - (ref ** 2).sum(axis=0)).max() <= TOL
    # the lens scene without the flag is the plain scene, wavefront kernels included
    with Renderer(sc) as q:
        assert same(pin, q.render(12, 12, 2, 3, 5, out_f64=True, aa=True))


# 6 ---------------------------------------------------- the R = 0 equalities --
def test_radius_zero_and_the_flag_off(cornell, plain, RA):
    aa = plain.render(12, 12, 8, 3, 9, out_f64=True, aa=True, lanes_per_pixel=4)
    pin = plain.render(12, 12, 8, 3, 9, out_f64=True, lanes_per_pixel=4)
    with Renderer(cornell, lens=(0.0, -24.0)) as r0:
        assert r0.params(12, 12).flags & PT_FLAG_LENS
        assert same(r0.render(12, 12, 8, 3, 9, out_f64=True, aa=True, lanes_per_pixel=4), aa)
        assert same(r0.render(12, 12, 8, 3, 9, out_f64=True, lanes_per_pixel=4), pin)
    # a lens scene without the flag: the plain scene's frames
    assert same(RA.render(12, 12, 8, 3, 9, out_f64=True, aa=True, lanes_per_pixel=4, lens=False), aa)
    assert same(RA.render(12, 12, 8, 3, 9, out_f64=True, lanes_per_pixel=4, lens=False), pin)


# 7 ----------------------------------------------------------- MultiRenderer --
def test_multirenderer_on_one_device_two_bands(cornell, RA, refA):
    m = MultiRenderer(cornell, [0, 0], lens=(A["R"], A["zf"]))
    try:
        assert m.lens == (A["R"], A["zf"]) and all(r.lens == m.lens for r in m.renderers)
        two = m.render(12, 12, 8, 3, 9, out_f64=True, aa=True, lanes_per_pixel=4)
        res = m.render_adaptive(12, 12, 8, 3, 9, tol=0.0, min_spp=8, step_spp=4, aa=True,
                                lanes_per_pixel=4, moments=True)
    finally:
        m.close()
    assert same(two, RA.render(12, 12, 8, 3, 9, out_f64=True, aa=True, lanes_per_pixel=4))
    assert mean_err(two, refA, 8) <= TOL
    assert np.abs(res.S - refA.sum(axis=0)).max() <= TOL
    # a lens handle and a lens-free one are not one scene
    m = MultiRenderer(cornell, [0])
    try:
        with Renderer(cornell, device=0, lens=(0.25, -24.0)) as other:
            m.renderers.append(other)
            with pytest.raises(_native.NativeError, match=r"\(-1\): .*another scene"):
                m.render(12, 12, 2, 3, 9)
            m.renderers.pop()
    finally:
        m.close()


# 8 -------------------------------------------------------------- validation --
def test_validation_and_the_handle_afterwards(cornell, plain, RA):
    before = RA.render(12, 12, 4, 3, 9, out_f64=True, aa=True)
    p = RA.params(12, 12, 4, 3, 9, aa=True)
    for flag in (PT_FLAG_COUNT, PT_FLAG_WALK_COUNT, PT_FLAG_KERNEL_TIMES):
        with pytest.raises(_native.NativeError, match=r"\(-1\): .*PT_FLAG_LENS"):
            RA.render_params(with_flags(p, flag))
    with Accumulator(RA, 12, 12) as acc:
        for flag in (PT_FLAG_WALK_COUNT, PT_FLAG_KERNEL_TIMES):
            with pytest.raises(_native.NativeError, match=r"\(-1\): .*PT_FLAG_LENS"):
                acc.render(with_flags(p, flag), make_adapt(0.0, 4, 4, 4))
    # the flag on a scene without a lens
    q = plain.params(12, 12, 4, 3, 9)
    with pytest.raises(_native.NativeError, match=r"\(-1\): .*pt_scene_create_lens"):
        plain.render_params(with_flags(q, PT_FLAG_LENS))
    with Accumulator(plain, 12, 12) as acc:
        with pytest.raises(_native.NativeError, match=r"\(-1\): .*pt_scene_create_lens"):
            acc.render(with_flags(q, PT_FLAG_LENS), make_adapt(0.0, 4, 4, 4))
    with pytest.raises(ValueError, match="created with a lens"):
        plain.render(12, 12, 4, 3, 9, lens=True)
    # lenses the scene entry refuses
    ez = float(plain.packed.eye[2])
    for lens in ((-0.1, -24.0), (float("nan"), -24.0), (0.5, float("inf")), (0.5, ez), (0.5, 2 * ez)):
        with pytest.raises(_native.NativeError, match=r"\(-1\): .*lens"):
            Renderer(cornell, lens=lens)
    assert same(RA.render(12, 12, 4, 3, 9, out_f64=True, aa=True), before)
    assert same(plain.render(12, 12, 4, 3, 9, out_f64=True), RA.render(12, 12, 4, 3, 9, out_f64=True, lens=False))


# 9 --------------------------------------------------------------------- CLI --
def test_command_line(RA, tmp_path, capsys):
    """--aperture / --focus-z alone, with --aa, --chunk-spp / --checkpoint,
    --noise --denoise and --local-devices: the frames the library calls give."""
    from conftest import CORNELL
    from pathtracerpython_amd import main as cli
    lens = ["--aperture", str(A["R"]), "--focus-z", str(A["zf"])]
    base = [CORNELL, "-r", "4", "-b", "2", "--size", "12", "12", "--seed", "9", "--aa"] + lens
    want = RA.render(12, 12, 4, 2, 9, out_f64=True, aa=True)
    assert same(np.asarray(cli.main(base), dtype=np.float64), want)
    assert same(np.asarray(cli.main([a for a in base if a != "--aa"]), dtype=np.float64),
                RA.render(12, 12, 4, 2, 9, out_f64=True))
    ck = str(tmp_path / "cli.npz")
    fb = cli.main(base + ["--chunk-spp", "2", "--checkpoint", ck])
    assert np.abs(fb - want).max() <= 1e-14
    with pytest.raises(ValueError, match="another render"):   # the file is a lens run's
        cli.main(base[:-4] + ["--chunk-spp", "2", "--checkpoint", ck])
    res = render_adaptive(RA, 12, 12, 4, 2, 9, tol=0.05, min_spp=2, step_spp=2, aa=True, denoise=True)
    noise = ["--noise", "0.05", "--min-spp", "2", "--step-spp", "2", "--denoise"]
    assert same(cli.main(base + noise), res.denoised)
    assert np.abs(cli.main(base + noise + ["--local-devices", "1"]) - res.denoised).max() <= 1e-12
    assert same(np.asarray(cli.main(base + ["--local-devices", "1"]), dtype=np.float64), want)
    with pytest.raises(SystemExit, match="--devices 1"):
        cli.main(base + ["--devices", "2"])
    capsys.readouterr()
