"""The thin lens on BVH scenes through the wavefront kernels (pt_shade_lens.hip
k_wf_shade_lens / k_wf_shade_list_lens: a primary query per sample from the
sample's lens point, in the slot's own record; render_wavefront with
PT_FLAG_LENS): which path a launch takes (pt_last_launch_info), the frames and
accumulator passes against the single kernel (megakernel=True) bit for bit and
against the oracle's per-sample colours through the lens (tests/lens_ref.py on
the mesh scene), splits and ragged launches, sample ranges, the R = 0
equalities, the walk stack's bound, bands, the buffers a scene handle shares,
validation and the command line.  Host-side cases:
tests/test_lens_wavefront_host.py."""
import os
import sys

import numpy as np
import pytest

import lens_ref
import lens_wf_ref as ref
from conftest import CORNELL, GOLDEN
from deep_scenes import COMB_ABOVE, COMB_BELOW, comb_scene, sliver_scene
from pathtracerpython_amd import _native
from pathtracerpython_amd._abi import (PT_FLAG_AA, PT_FLAG_FORCE_F64, PT_FLAG_KERNEL_TIMES, PT_FLAG_LENS,
                                       PT_FLAG_MEGAKERNEL, PT_FLAG_OUT_F64, PT_FLAG_RR, PT_FLAG_WALK_COUNT,
                                       PT_PATH_NONE, PT_PATH_SINGLE, PT_PATH_WAVEFRONT, make_adapt, with_flags)
from pathtracerpython_amd.adaptive import Accumulator, render_adaptive, run_passes
from pathtracerpython_amd.render import MultiRenderer, Renderer

pytestmark = pytest.mark.gpu

TOL = 1e-12
FLOOR = 0.01
A, B = ref.A, ref.B
W = H = 12
BOUNCES, SEED = ref.BOUNCES, ref.SEED
REFUSED = r"\(-1\): .*PT_FLAG_LENS"


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else a.dtype)


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def same_bits(a, b):
    return all(same(a[k], b[k]) for k in ("S", "Q", "n"))


def gpu():
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"


@pytest.fixture(scope="module")
def sc(mesh_golden):
    gpu()
    return ref.use_scene(mesh_golden[0])


@pytest.fixture(scope="module")
def RA(sc):
    with Renderer(sc, lens=(A["R"], A["zf"])) as r:
        yield r


@pytest.fixture(scope="module")
def RB(sc):
    with Renderer(sc, lens=(B["R"], B["zf"])) as r:
        yield r


@pytest.fixture(scope="module")
def plain(sc):
    with Renderer(sc) as r:
        yield r


@pytest.fixture(scope="module")
def frames(sc):
    """{case: the oracle's per-sample frames [n, H, W, 3]} (17 of A, 8 of B),
    the restart's branches asserted (tests/lens_wf_ref.py)."""
    return {c: ref.frames(c) for c in ("A", "B")}


def mean_err(fb, fr, spp, begin=0):
    return float(np.abs(fb - fr[begin:begin + spp].sum(axis=0) / spp).max())


def both(r, *a, **kw):
    """(wavefront, single kernel) f64 frames of one render through r's lens,
    the path of each launch asserted."""
    wf = r.render(*a, out_f64=True, **kw)
    assert r.last_launch()["path"] == PT_PATH_WAVEFRONT
    mk = r.render(*a, out_f64=True, megakernel=True, **kw)
    assert r.last_launch()["path"] == PT_PATH_SINGLE
    return wf, mk


def one_pass(r, frame, spp, aa, flags=0):
    """One whole pass (every pixel, spp samples): the accumulator's S, Q, n and
    the launch record."""
    w, h, b, seed = frame
    p = with_flags(r.params(w, h, spp, b, seed, aa=aa), flags)
    with Accumulator(r, w, h) as acc:
        acc.render(p, make_adapt(0.0, spp, spp, spp))
        return acc.read(S=True, Q=True, n=True), r.last_launch()


def run(r, frame, rule, tol, aa, megakernel=False):
    """A whole adaptive run through the lens: (S, Q, n dict, passes)."""
    w, h, b, seed = frame
    mn, mx, st = rule
    p = r.params(w, h, mx, b, seed, megakernel=megakernel, aa=aa)
    with Accumulator(r, w, h) as acc:
        passes = run_passes(acc, p, make_adapt(tol, mx, mn, st, FLOOR))
        return acc.read(S=True, Q=True, n=True), passes


# 1 ---------------------------------------------------------- the path ran --
def test_which_path_a_launch_takes(sc, RA, plain, cornell):
    """4 samples over 4 slots, 3 bounces through the lens: a sample is its
    primary query and three bounce steps, so 1 x (3 + 1) + 2 shade launches;
    the centre-ray render's primary query is shared: 1 x 3 + 2."""
    with Renderer(sc, lens=(A["R"], A["zf"])) as r:
        assert r.last_launch() == {"path": PT_PATH_NONE, "steps": 0, "lanes_per_pixel": 0, "flags": 0}
        r.render(12, 12, 4, 3, 5, aa=True, lanes_per_pixel=4)
        assert r.last_launch() == {"path": PT_PATH_WAVEFRONT, "steps": 6, "lanes_per_pixel": 4,
                                   "flags": PT_FLAG_LENS | PT_FLAG_AA}
        r.render(12, 12, 4, 3, 5, lanes_per_pixel=4)       # without PT_FLAG_AA: the same step count
        assert r.last_launch() == {"path": PT_PATH_WAVEFRONT, "steps": 6, "lanes_per_pixel": 4,
                                   "flags": PT_FLAG_LENS}
        r.render(12, 12, 4, 3, 5, aa=True, lanes_per_pixel=4, row_begin=3, row_end=3)   # no rows: no launch
        assert r.last_launch()["flags"] == PT_FLAG_LENS
        for kw in (dict(megakernel=True), dict(force_f64=True)):
            r.render(12, 12, 4, 3, 5, aa=True, lanes_per_pixel=4, out_f64=True, **kw)
            got = r.last_launch()
            assert (got["path"], got["steps"], got["lanes_per_pixel"]) == (PT_PATH_SINGLE, 1, 4)
            assert got["flags"] & PT_FLAG_LENS and got["flags"] & PT_FLAG_OUT_F64
        # an accumulator pass likewise
        d, got = one_pass(r, (12, 12, 3, 5), 4, True)
        assert (got["path"], got["steps"], got["lanes_per_pixel"]) == (PT_PATH_WAVEFRONT, 6, 4)
        assert got["flags"] == PT_FLAG_LENS | PT_FLAG_AA and (d["n"] == 4).all()
        for flag in (PT_FLAG_MEGAKERNEL, PT_FLAG_FORCE_F64):
            _, got = one_pass(r, (12, 12, 3, 5), 4, True, flag)
            assert (got["path"], got["steps"]) == (PT_PATH_SINGLE, 1)
        # a centre-ray render of the lens scene
        r.render(12, 12, 4, 3, 5, lanes_per_pixel=4, lens=False)
        assert r.last_launch() == {"path": PT_PATH_WAVEFRONT, "steps": 5, "lanes_per_pixel": 4, "flags": 0}
    plain.render(12, 12, 4, 3, 5, lanes_per_pixel=4)
    assert plain.last_launch() == {"path": PT_PATH_WAVEFRONT, "steps": 5, "lanes_per_pixel": 4, "flags": 0}
    plain.render(12, 12, 8, 3, 5, lanes_per_pixel=2, aa=True)
    assert plain.last_launch() == {"path": PT_PATH_WAVEFRONT, "steps": 4 * 4 + 2, "lanes_per_pixel": 2,
                                   "flags": PT_FLAG_AA}
    with Renderer(cornell, lens=(A["R"], A["zf"])) as c:      # no BVH
        c.render(12, 12, 4, 3, 9, aa=True, lanes_per_pixel=4)
        got = c.last_launch()
        assert (got["path"], got["steps"], got["lanes_per_pixel"]) == (PT_PATH_SINGLE, 1, 4)


# 2 ------------------------------------------------------------------ frames --
@pytest.mark.parametrize("spp", [2, 8])
@pytest.mark.parametrize("case", ["A", "B"])
def test_frames(RA, RB, frames, case, spp):
    r, aa = (RA, True) if case == "A" else (RB, False)
    fb, mk = both(r, W, H, spp, BOUNCES, SEED, aa=aa)
    assert same(fb, mk)
    e = mean_err(fb, frames[case], spp)
    print(f"{case} 12x12x{spp} wavefront lens frame vs oracle: {e:.3e}")
    assert e <= TOL
    f32 = r.render(W, H, spp, BOUNCES, SEED, aa=aa)
    e32 = mean_err(f32.astype(np.float64), frames[case], spp)
    print(f"{case} 12x12x{spp} f32 frame vs oracle: {e32:.3e}")
    assert f32.dtype == np.float32 and e32 <= 1e-6
    if case == "A":      # the lens is on: not the pinhole antialiased frame
        assert np.abs(fb - r.render(W, H, spp, BOUNCES, SEED, out_f64=True, aa=True, lens=False)).max() > 1e-3


# 3 ------------------------------------------------ splits, ragged launches --
@pytest.mark.parametrize("lanes", [1, 2, 4])
def test_slots_per_pixel(RA, sc, lanes):
    """7 x 5 at 8 / 5 / 3 samples (lanes_per_pixel <= spp); 5 samples on 4
    slots: unequal shares."""
    fr = ref.frames_small("7x5")
    for spp in (8, 5, 3):
        if lanes > spp:
            continue
        fb, mk = both(RA, 7, 5, spp, 3, 5, aa=True, lanes_per_pixel=lanes)
        assert fb.shape == (5, 7, 3) and same(fb, mk)
        assert mean_err(fb, fr, spp) <= TOL


@pytest.mark.parametrize("lanes", [16, 64])
def test_wide_pixels(RA, sc, lanes):
    fr = ref.frames_small("6x6")
    fb, mk = both(RA, 6, 6, 64, 2, 5, aa=True, lanes_per_pixel=lanes)
    assert same(fb, mk)
    assert mean_err(fb, fr, 64) <= TOL


@pytest.mark.parametrize("w,h", [(5, 7), (1, 1), (3, 1)])
def test_partial_last_shade_block(RA, RB, w, h):
    for lanes in (1, 4):
        for r, aa in ((RA, True), (RB, False)):
            fb, mk = both(r, w, h, 4, 3, 5, aa=aa, lanes_per_pixel=lanes)
            assert fb.shape == (h, w, 3) and same(fb, mk)


# 4 ----------------------------------------- RR, zero bounces, one bounce --
def test_russian_roulette_no_bounces_and_one_bounce(RA, sc):
    fr = lens_ref.to_image(ref.samples("A", 8, 8, 4, 4, PT_FLAG_RR, 1), 8, 8)
    fb, mk = both(RA, 8, 8, 4, 4, SEED, aa=True, rr=True, rr_depth=1)
    assert same(fb, mk) and mean_err(fb, fr, 4) <= TOL
    fb, mk = both(RA, 8, 8, 4, 0, SEED, aa=True)
    assert same(fb, mk) and not fb.any()
    assert RA.render(8, 8, 4, 0, SEED, aa=True) is not None and RA.last_launch()["steps"] == 1 * (0 + 1) + 2
    fr = lens_ref.to_image(ref.samples("A", 8, 8, 1, 4, 0, 3), 8, 8)
    fb, mk = both(RA, 8, 8, 4, 1, SEED, aa=True)
    assert same(fb, mk) and fb.any() and mean_err(fb, fr, 4) <= TOL
    for b in (0, 1):
        d, _ = one_pass(RA, (8, 8, b, SEED), 4, True)
        m, _ = one_pass(RA, (8, 8, b, SEED), 4, True, PT_FLAG_MEGAKERNEL)
        assert same_bits(d, m) and (d["n"] == 4).all()


# 5 ------------------------------------------------------------ sample ranges --
def test_sample_ranges(RA, frames):
    fb, mk = both(RA, W, H, 5, BOUNCES, SEED, aa=True, sample_begin=3)
    assert same(fb, mk)
    e = mean_err(fb, frames["A"], 5, begin=3)
    print(f"samples 3..7 vs oracle: {e:.3e}")
    assert e <= TOL


# 6 ------------------------------------------------------------- accumulator --
@pytest.mark.parametrize("case", ["A", "B"])
def test_one_whole_pass(RA, RB, frames, case):
    r, aa = (RA, True) if case == "A" else (RB, False)
    spp = 8
    d, got = one_pass(r, (W, H, BOUNCES, SEED), spp, aa)
    m, gm = one_pass(r, (W, H, BOUNCES, SEED), spp, aa, PT_FLAG_MEGAKERNEL)
    assert got["path"] == PT_PATH_WAVEFRONT and gm["path"] == PT_PATH_SINGLE
    assert same_bits(d, m) and (d["n"] == spp).all()
    ws, wq = ref.sums(frames[case][:spp])
    dS, dQ = float(np.abs(d["S"] - ws).max()), float(np.abs(d["Q"] - wq).max())
    print(f"{case}: |S - oracle| = {dS:.3e}, |Q - oracle| = {dQ:.3e}")
    assert dS <= TOL and dQ <= TOL


def test_adaptive_run_equals_the_single_kernel(RA):
    frame = (W, H, BOUNCES, SEED)
    d, passes = run(RA, frame, (3, 17, 5), 0.05, True)
    assert RA.last_launch()["path"] == PT_PATH_WAVEFRONT
    mk, passes_mk = run(RA, frame, (3, 17, 5), 0.05, True, megakernel=True)
    assert RA.last_launch()["path"] == PT_PATH_SINGLE
    assert same_bits(d, mk) and passes == passes_mk and len(passes) >= 2
    assert len(np.unique(d["n"])) >= 2 and d["n"].max() <= 17


def test_accumulator_refuses_mixed_passes(RA):
    adapt = make_adapt(0.0, 4, 4, 2)      # every pixel: two passes of two samples
    off = RA.params(8, 8, 4, 2, 9, lens=False)
    on = RA.params(8, 8, 4, 2, 9)
    with Accumulator(RA, 8, 8) as acc:
        acc.render(on, adapt)
        assert RA.last_launch()["path"] == PT_PATH_WAVEFRONT
        with pytest.raises(_native.NativeError, match=REFUSED):
            acc.render(off, adapt)
        acc.render(on, adapt)                               # the handle is still usable
        assert (acc.read(n=True)["n"] == 4).all()
        acc.reset()
        acc.render(off, adapt)                              # after a reset either value
        with pytest.raises(_native.NativeError, match=REFUSED):
            acc.render(on, adapt)


# 7 ---------------------------------------------------- the R = 0 equalities --
def test_radius_zero_on_the_device(sc, plain):
    aa = plain.render(W, H, 8, BOUNCES, SEED, out_f64=True, aa=True, lanes_per_pixel=4)
    pin = plain.render(W, H, 8, BOUNCES, SEED, out_f64=True, lanes_per_pixel=4)
    assert plain.last_launch()["path"] == PT_PATH_WAVEFRONT and not same(aa, pin)
    with Renderer(sc, lens=(0.0, -24.0)) as r0:
        got = r0.render(W, H, 8, BOUNCES, SEED, out_f64=True, aa=True, lanes_per_pixel=4)
        assert r0.last_launch()["path"] == PT_PATH_WAVEFRONT and r0.last_launch()["flags"] & PT_FLAG_LENS
        assert same(got, aa)
        got = r0.render(W, H, 8, BOUNCES, SEED, out_f64=True, lanes_per_pixel=4)
        assert r0.last_launch()["path"] == PT_PATH_WAVEFRONT and r0.last_launch()["flags"] & PT_FLAG_LENS
        assert same(got, pin)


# 8 -------------------------------------------------------------- walk stack --
@pytest.mark.parametrize("comb,path", [(COMB_BELOW, PT_PATH_WAVEFRONT), (COMB_ABOVE, PT_PATH_SINGLE)],
                         ids=["qstack48", "qstack49"])
def test_comb_scenes_at_the_walk_stack_bound(tmp_path, comb, path):
    gpu()
    with Renderer(comb_scene(tmp_path, *comb), lens=(0.25, -24.0)) as r:
        fb = r.render(20, 16, 2, 4, 9, out_f64=True, aa=True)
        assert r.last_launch()["path"] == path
        assert fb.any() and same(fb, r.render(20, 16, 2, 4, 9, out_f64=True, aa=True, megakernel=True))
        d, got = one_pass(r, (20, 16, 4, 9), 2, True)
        m, _ = one_pass(r, (20, 16, 4, 9), 2, True, PT_FLAG_MEGAKERNEL)
        assert got["path"] == path and same_bits(d, m) and d["S"].any()


def test_sliver_scene_through_the_spilled_stacks(tmp_path):
    gpu()
    with Renderer(sliver_scene(tmp_path), lens=(0.25, -24.0)) as r:
        for aa in (True, False):
            fb, mk = both(r, 16, 16, 2, 4, 9, aa=aa)
            assert same(fb, mk) and fb.any()
        d, _ = one_pass(r, (16, 16, 4, 9), 2, True)
        m, _ = one_pass(r, (16, 16, 4, 9), 2, True, PT_FLAG_MEGAKERNEL)
        assert same_bits(d, m)


# 9 ------------------------------------------------- bands, shared buffers --
def test_multirenderer_on_one_device_two_bands(sc, RA):
    kw = dict(max_spp=8, bounces=BOUNCES, seed=SEED, tol=0.05, min_spp=4, step_spp=4, floor=FLOOR,
              lanes_per_pixel=4, aa=True, moments=True)
    one_fb = RA.render(W, H, 8, BOUNCES, SEED, out_f64=True, aa=True, lanes_per_pixel=4)
    one = render_adaptive(RA, W, H, **kw)
    m = MultiRenderer(sc, [0, 0], lens=(A["R"], A["zf"]))
    try:
        two_fb = m.render(W, H, 8, BOUNCES, SEED, out_f64=True, aa=True, lanes_per_pixel=4)
        assert [r.last_launch()["path"] for r in m.renderers] == [PT_PATH_WAVEFRONT] * 2
        two = m.render_adaptive(W, H, **kw)
    finally:
        m.close()
    assert same(two_fb, one_fb)
    for k in ("S", "Q", "counts", "err"):
        assert same(getattr(one, k), getattr(two, k)), k


def test_one_handle_runs_every_form_in_turn(sc):
    """A centre-ray render, an antialiased one, a lens render and a lens list
    pass on one handle: each finds the buffers the one before left, and equals
    its result on a fresh handle."""
    lens = (A["R"], A["zf"])
    jobs = [lambda r: r.render(W, H, 6, BOUNCES, SEED, out_f64=True, lens=False),
            lambda r: r.render(9, 4, 5, BOUNCES, SEED, out_f64=True, aa=True, lens=False),
            lambda r: r.render(W, H, 5, BOUNCES, SEED, out_f64=True, aa=True),
            lambda r: one_pass(r, (7, 5, 3, 11), 4, True)[0]]
    fresh = []
    for job in jobs:
        with Renderer(sc, lens=lens) as r:
            fresh.append(job(r))
    with Renderer(sc, lens=lens) as r:
        got = [job(r) for job in jobs]
    for g, f in zip(got[:3], fresh[:3]):
        assert same(g, f)
    assert same_bits(got[3], fresh[3]) and not same(fresh[0], fresh[2])


# 10 ------------------------------------------------------------- validation --
def test_validation_and_the_handle_afterwards(RA):
    before = RA.render(W, H, 4, BOUNCES, SEED, out_f64=True, aa=True)
    p = RA.params(W, H, 4, BOUNCES, SEED, aa=True, out_f64=True)
    for flag in (PT_FLAG_WALK_COUNT, PT_FLAG_KERNEL_TIMES):
        with pytest.raises(_native.NativeError, match=REFUSED):
            RA.render_params(with_flags(p, flag))
        with Accumulator(RA, W, H) as acc:
            with pytest.raises(_native.NativeError, match=REFUSED):
                acc.render(with_flags(RA.params(W, H, 4, BOUNCES, SEED, aa=True), flag), make_adapt(0.0, 4, 4, 4))
    assert same(RA.render(W, H, 4, BOUNCES, SEED, out_f64=True, aa=True), before)
    assert RA.last_launch()["path"] == PT_PATH_WAVEFRONT


# 11 ----------------------------------------------------------- command line --
def test_command_line(RA, tmp_path, capsys):
    sys.path.insert(0, GOLDEN)
    import mesh_scene as ms
    from pathtracerpython_amd import main as cli
    sdl = ms.write_mesh_scene(str(tmp_path), os.path.dirname(CORNELL))
    argv = [sdl, "-r", "4", "-b", "2", "--size", "12", "12", "--seed", "5", "--aa", "--aperture", "0.25",
            "--focus-z", "-24"]
    want = RA.render(12, 12, 4, 2, 5, out_f64=True, aa=True)
    assert RA.last_launch()["path"] == PT_PATH_WAVEFRONT
    assert same(np.asarray(cli.main(argv), dtype=np.float64), want)
    capsys.readouterr()
