"""Caller-supplied rays on BVH scenes through the wavefront kernels
(pt_shade_rays.hip k_wf_shade_rays / k_wf_primary_rays / k_wf_final_rays;
render_wavefront with a ray batch): which path a launch takes
(pt_last_launch_info), the wavefront result against the single ray kernel
(single_kernel=True, PT_FLAG_RAYS_SINGLE) bit for bit in mean, S and Q,
against the oracle's per-sample colours (tests/rays_ref.py), the frame's own
rays against Renderer.render, the independence of the batch, the buffers a
scene handle shares, the device entry, the refusals and the command line.
Host-side cases: tests/test_rays_wavefront_host.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import rays_ref
from conftest import CORNELL, GOLDEN
from deep_scenes import COMB_ABOVE, COMB_BELOW, comb_scene
from pathtracerpython_amd import _native, cameras
from pathtracerpython_amd._abi import (PT_FLAG_KERNEL_TIMES, PT_FLAG_OUT_F64, PT_FLAG_RAYS_SINGLE, PT_FLAG_WALK_COUNT,
                                       PT_PATH_SINGLE, PT_PATH_WAVEFRONT, PtStats, make_adapt, make_params,
                                       make_rays, with_flags)
from pathtracerpython_amd.adaptive import Accumulator
from pathtracerpython_amd.render import MultiRenderer, Renderer

pytestmark = pytest.mark.gpu

TOL, TOL32 = 1e-12, 1e-6
# (n_rays, spp, bounces, rr_depth or None, sample_begin): tests/test_rays_wavefront_host.py's matrix
MATRIX = ((1, 1, 3, None, 0), (63, 5, 3, None, 0), (64, 8, 3, None, 0), (65, 8, 1, None, 0), (257, 1, 3, None, 0),
          (64, 5, 0, None, 0), (65, 8, 3, 1, 0), (63, 8, 3, None, 5))
ORACLE = (("mesh", 64, 8, 3, None, 0), ("mesh", 257, 1, 3, None, 0), ("multi", 63, 5, 3, None, 0),
          ("mesh", 16, 5, 3, 1, 0), ("mesh", 16, 5, 3, None, 5))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else a.dtype)


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def gpu():
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"


def mid(c):
    return "n%d-spp%d-b%d%s%s" % (c[0], c[1], c[2], "" if c[3] is None else "-rr%d" % c[3],
                                  "-s%d" % c[4] if c[4] else "")


@pytest.fixture(scope="module")
def benches(tmp_path_factory, cornell, mesh_golden):
    """name -> (rays_ref.Bench, Renderer with the bench's box, Renderer without)."""
    gpu()
    made = {}

    def get(name):
        if name not in made:
            b = rays_ref.Bench(rays_ref.make_scene(name, tmp_path_factory.mktemp(name), cornell, mesh_golden))
            made[name] = (b, Renderer(b.scene, ray_box=(b.box[:3], b.box[3:])), Renderer(b.scene))
        return made[name]
    yield get
    for _, r, q in made.values():
        r.close()
        q.close()


def kw_of(spp, bounces, rr_depth, s0):
    return dict(spp=spp, bounces=bounces, seed=9, rr=rr_depth is not None,
                rr_depth=3 if rr_depth is None else rr_depth, sample_begin=s0)


def both(r, o, d, keys, **kw):
    """(wavefront, single kernel) results of one launch each, the path of each asserted."""
    wf = r.render_rays(o, d, keys, **kw)
    assert r.last_launch()["path"] == PT_PATH_WAVEFRONT
    sk = r.render_rays(o, d, keys, single_kernel=True, **kw)
    assert r.last_launch()["path"] == PT_PATH_SINGLE
    return wf, sk


# 1 ---------------------------------------------------------- the path ran --
def test_which_path_a_launch_takes(benches, tmp_path):
    """8 samples over 4 slots, 3 bounces: the primary query is the record's, so
    2 x 3 + 2 shade launches."""
    b, r, _ = benches("mesh")
    n = 65
    kw = dict(spp=8, bounces=3, seed=9, lanes_per_pixel=4)
    r.render_rays(b.o[:n], b.d[:n], b.keys[:n], **kw)
    assert r.last_launch() == {"path": PT_PATH_WAVEFRONT, "steps": 2 * 3 + 2, "lanes_per_pixel": 4,
                               "flags": PT_FLAG_OUT_F64}
    r.render_rays(b.o[:n], b.d[:n], b.keys[:n], single_kernel=True, **kw)
    assert r.last_launch() == {"path": PT_PATH_SINGLE, "steps": 1, "lanes_per_pixel": 4,
                               "flags": PT_FLAG_OUT_F64 | PT_FLAG_RAYS_SINGLE}
    r.render_rays(b.o[:n], b.d[:n], b.keys[:n], force_f64=True, **kw)
    assert r.last_launch()["path"] == PT_PATH_SINGLE
    c, rc, _ = benches("cornell")
    rc.render_rays(c.o[:n], c.d[:n], c.keys[:n], **kw)
    assert rc.last_launch()["path"] == PT_PATH_SINGLE and rc.last_launch()["steps"] == 1
    for comb, path in ((COMB_BELOW, PT_PATH_WAVEFRONT), (COMB_ABOVE, PT_PATH_SINGLE)):
        d = tmp_path / ("q%d" % path)
        d.mkdir()
        with Renderer(comb_scene(d, *comb)) as q:
            got = q.render_rays(b.o[:n], b.d[:n], b.keys[:n], moments=True, **kw)
            assert q.last_launch()["path"] == path
            want = q.render_rays(b.o[:n], b.d[:n], b.keys[:n], moments=True, single_kernel=True, **kw)
            assert got[0].any() and all(same(x, y) for x, y in zip(got, want))


# 2 ------------------------------------------- wavefront = single, bitwise --
@pytest.mark.parametrize("name", ["mesh", "multi"])
@pytest.mark.parametrize("case", MATRIX, ids=mid)
def test_wavefront_is_the_single_kernel_bit_for_bit(benches, case, name):
    """Mean, S and Q; boxed and plain (the plain scene's frame leaves more
    origins to the f64 primary); the library's lane count, 1 and 4."""
    n, spp, bounces, rr_depth, s0 = case
    b, boxed, plain = benches(name)
    kw = kw_of(spp, bounces, rr_depth, s0)
    for r in (boxed, plain):
        for lanes in (0, 1, 4):
            if lanes > spp:
                continue
            wf, sk = both(r, b.o[:n], b.d[:n], b.keys[:n], lanes_per_pixel=lanes, **kw)
            assert same(wf, sk)
            wf, sk = both(r, b.o[:n], b.d[:n], b.keys[:n], lanes_per_pixel=lanes, moments=True, **kw)
            assert all(same(x, y) for x, y in zip(wf, sk)) and same(wf[0], wf[1] / spp)
            assert wf[0].any() if bounces > 0 else not (wf[0].any() or wf[1].any() or wf[2].any())
    wf, sk = both(boxed, b.o[:n], b.d[:n], b.keys[:n], out_f64=False, **kw)
    assert wf.dtype == np.float32 and same(wf, sk)


def test_f32_output_against_the_oracle(benches):
    name, n, spp, bounces, rr_depth, s0 = ORACLE[0]
    b, boxed, _ = benches(name)
    want = b.samples(n, bounces, rr_depth, s0, spp)
    f32 = boxed.render_rays(b.o[:n], b.d[:n], b.keys[:n], out_f64=False, **kw_of(spp, bounces, rr_depth, s0))
    assert boxed.last_launch()["path"] == PT_PATH_WAVEFRONT and f32.dtype == np.float32
    assert float(np.abs(f32 - want.sum(axis=0) / spp).max()) <= TOL32


# 3 ----------------------------------------------------------- the oracle --
@pytest.mark.parametrize("case", ORACLE, ids=rays_ref.case_id)
def test_oracle_parity(benches, case):
    """Every record's mean, S and Q within 1e-12 of the oracle, none excluded,
    through the wavefront kernels; with and without the box."""
    name, n, spp, bounces, rr_depth, s0 = case
    b, boxed, plain = benches(name)
    esc, light, spec = rays_ref.first_hits(b.pk, b.o, b.d)
    assert esc >= 1 and light >= 1 and spec >= 1
    assert b.outside[:n].any() and not b.outside[:n].all()
    want = b.samples(n, bounces, rr_depth, s0, spp)
    mean, S, Q = want.sum(axis=0) / spp, want.sum(axis=0), (want ** 2).sum(axis=0)
    kw = kw_of(spp, bounces, rr_depth, s0)
    for r in (boxed, plain):
        for lanes in (1, 4):
            if lanes > spp:
                continue
            rgb = r.render_rays(b.o[:n], b.d[:n], b.keys[:n], lanes_per_pixel=lanes, **kw)
            assert r.last_launch()["path"] == PT_PATH_WAVEFRONT
            g, gS, gQ = r.render_rays(b.o[:n], b.d[:n], b.keys[:n], lanes_per_pixel=lanes, moments=True, **kw)
            assert r.last_launch()["path"] == PT_PATH_WAVEFRONT
            errs = [float(np.abs(x - y).max()) for x, y in ((rgb, mean), (g, mean), (gS, S), (gQ, Q))]
            print(f"{rays_ref.case_id(case)} {'box' if r is boxed else 'plain'} lanes {lanes}: mean {errs[0]:.3e} "
                  f"/ {errs[1]:.3e}, S {errs[2]:.3e}, Q {errs[3]:.3e}")
            assert max(errs) <= TOL


# 4 ------------------------------------------------------ the frame's rays --
def test_frame_of_the_mesh_scene_three_ways(benches):
    """render_rays (wavefront) = Renderer.render (wavefront) =
    render(megakernel=True), bit for bit, 12 x 12, 8 spp, 1 and 4 lanes."""
    b, _, r = benches("mesh")
    o, d, keys = cameras.scene_camera_rays(b.scene, 12, 12)
    for lanes in (1, 4):
        rgb = r.render_rays(o, d, keys, spp=8, bounces=3, seed=9, lanes_per_pixel=lanes)
        assert r.last_launch()["path"] == PT_PATH_WAVEFRONT
        frame = r.render(12, 12, 8, 3, 9, out_f64=True, lanes_per_pixel=lanes)
        assert r.last_launch()["path"] == PT_PATH_WAVEFRONT
        mk = r.render(12, 12, 8, 3, 9, out_f64=True, megakernel=True, lanes_per_pixel=lanes)
        assert r.last_launch()["path"] == PT_PATH_SINGLE
        assert frame.any() and same(frame, mk)
        assert same(np.ascontiguousarray(cameras.rays_to_image(rgb, 12, 12)), frame)


# 5 ------------------------------------------------------------- the batch --
def test_a_record_does_not_depend_on_its_batch(benches):
    """tests/test_gpu_rays.py's test on the mesh scene, every launch through
    the wavefront kernels: a permutation, two launches, padding, twins."""
    b, r, _ = benches("mesh")
    n = 65
    kw = dict(spp=8, bounces=3, seed=9, moments=True)
    for lanes in (1, 4):
        def go(sel):
            out = r.render_rays(b.o[sel], b.d[sel], b.keys[sel], lanes_per_pixel=lanes, **kw)
            assert r.last_launch()["path"] == PT_PATH_WAVEFRONT
            return out
        base = go(slice(0, n))
        perm = np.random.default_rng(3).permutation(n)
        sh, one, two = go(perm), go(slice(0, 20)), go(slice(20, n))
        pad = go(np.arange(n + 30)[::-1])
        for x, y, z, w, v in zip(base, sh, one, two, pad):
            assert same(x[perm], y)
            assert same(x, np.concatenate([z, w]))
            assert same(x, np.ascontiguousarray(v[::-1][:n]))
    twin = r.render_rays(b.o[[4, 4, 9]], b.d[[4, 4, 9]], b.keys[[4, 4, 9]], **kw)
    assert all(same(x[0], x[1]) for x in twin) and twin[0].any()


# 6 --------------------------------------------------- the shared buffers --
def test_one_handle_runs_frames_rays_and_a_list_pass_in_turn(benches):
    """A frame, a ray launch with more slots (the block regrows), the frame
    again, an adaptive list pass: each equals its result on a fresh handle."""
    b, _, _ = benches("mesh")
    n = 257

    def one_pass(r):
        with Accumulator(r, 7, 5) as acc:
            acc.render(r.params(7, 5, 4, 3, 11), make_adapt(0.0, 4, 4, 4))
            assert r.last_launch()["path"] == PT_PATH_WAVEFRONT
            return acc.read(S=True, Q=True, n=True)
    jobs = [lambda r: r.render(8, 8, 4, 3, 9, out_f64=True, lanes_per_pixel=1),
            lambda r: r.render_rays(b.o[:n], b.d[:n], b.keys[:n], spp=8, bounces=3, seed=9, lanes_per_pixel=8,
                                    moments=True),
            lambda r: r.render(8, 8, 4, 3, 9, out_f64=True, lanes_per_pixel=1),
            one_pass]
    fresh = []
    for job in jobs:
        with Renderer(b.scene) as r:
            fresh.append(job(r))
    with Renderer(b.scene) as r:
        got = [job(r) for job in jobs]
    assert same(got[0], fresh[0]) and same(got[2], fresh[2]) and fresh[0].any()
    assert all(same(x, y) for x, y in zip(got[1], fresh[1]))
    assert all(same(got[3][k], fresh[3][k]) for k in ("S", "Q", "n"))


# 7 ------------------------------------------------------ the device entry --
def test_device_entry_on_a_side_stream(benches):
    import torch
    b, r, _ = benches("mesh")
    n = 65
    rec = make_rays(b.o[:n], b.d[:n], b.keys[:n])
    want = r.render_rays(b.o[:n], b.d[:n], b.keys[:n], spp=8, bounces=3, seed=9, lanes_per_pixel=4, moments=True)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        rays = torch.from_numpy(np.frombuffer(rec.tobytes(), dtype=np.uint8).copy()).cuda()
        rgb = torch.zeros((n, 3), dtype=torch.float64, device="cuda")
        S, Q = torch.zeros_like(rgb), torch.zeros_like(rgb)
        p = make_params(1, 1, 8, 3, 9, PT_FLAG_OUT_F64, lanes_per_pixel=4)
        assert side.cuda_stream != 0
        _native.check(_native.lib().pt_radiance_device(r._h, C.c_void_p(rays.data_ptr()), n, C.byref(p),
                                                       C.c_void_p(rgb.data_ptr()), C.c_void_p(S.data_ptr()),
                                                       C.c_void_p(Q.data_ptr()), C.c_void_p(side.cuda_stream)),
                      "pt_radiance_device")
    side.synchronize()
    assert r.last_launch()["path"] == PT_PATH_WAVEFRONT and r.last_kernel_ms() > 0.0
    assert same(rgb.cpu().numpy(), want[0]) and same(S.cpu().numpy(), want[1]) and same(Q.cpu().numpy(), want[2])


# 8 ------------------------------------------------------------- refusals --
def test_refusals(benches):
    b, r, _ = benches("mesh")
    lib = _native.lib()
    p = r.params(8, 8, 4, 2, 9)
    with pytest.raises(_native.NativeError, match=r"\(-1\)"):
        r.render_params(with_flags(p, PT_FLAG_RAYS_SINGLE))
    with Accumulator(r, 8, 8) as acc:
        with pytest.raises(_native.NativeError, match=r"\(-1\)"):
            acc.render(with_flags(p, PT_FLAG_RAYS_SINGLE), make_adapt(0.0, 4, 4, 4))
    m = MultiRenderer(b.scene, [0, 0])
    try:
        out = np.zeros((8, 8, 3), dtype=np.float32)
        hs = (C.c_void_p * 2)(*[q._h.value for q in m.renderers])
        q = with_flags(m.renderers[0].params(8, 8, 4, 2, 9), PT_FLAG_RAYS_SINGLE)
        assert lib.pt_render_multi(hs, 2, C.byref(q), C.c_void_p(out.ctypes.data), C.byref(PtStats())) == -1
    finally:
        m.close()
    rec = make_rays(b.o[:4], b.d[:4], b.keys[:4])
    out = np.full((4, 3), -1.0)
    for flag in (PT_FLAG_WALK_COUNT, PT_FLAG_KERNEL_TIMES):
        q = make_params(1, 1, 2, 2, 9, PT_FLAG_OUT_F64 | flag)
        assert lib.pt_radiance(r._h, C.c_void_p(rec.ctypes.data), 4, C.byref(q), C.c_void_p(out.ctypes.data),
                               None, None) == -1
        assert "flag" in _native.last_error()
    assert (out == -1.0).all()
    # n_rays = 0 succeeds and leaves the last launch record untouched
    r.render(8, 8, 2, 2, 9, lanes_per_pixel=2)
    before = r.last_launch()
    q = make_params(1, 1, 2, 2, 9, PT_FLAG_OUT_F64)
    assert lib.pt_radiance(r._h, C.c_void_p(rec.ctypes.data), 0, C.byref(q), C.c_void_p(out.ctypes.data),
                           None, None) == 0
    assert r.last_launch() == before and before["path"] == PT_PATH_WAVEFRONT and (out == -1.0).all()


# 9 ------------------------------------------------------ the command line --
def test_cli_look_at_on_the_mesh_scene(mesh_golden, tmp_path, capsys):
    gpu()
    sys.path.insert(0, GOLDEN)
    import mesh_scene as ms
    from pathtracerpython_amd import main as cli
    sdl = ms.write_mesh_scene(str(tmp_path), os.path.dirname(CORNELL))
    out, raw = str(tmp_path / "look.png"), str(tmp_path / "look.npy")
    argv = [sdl, "--look-at", "2.5", "1.5", "4", "0", "0", "-24", "--fov", "30", "-r", "4", "-b", "2",
            "--seed", "9", "--size", "10", "8", "--out", out, "--save-raw", raw]
    fb = cli.main(argv)
    assert fb.shape == (8, 10, 3) and fb.dtype == np.float64 and same(np.load(raw), fb)
    o, d, keys = cameras.look_at_rays((2.5, 1.5, 4.0), (0.0, 0.0, -24.0), (0.0, 1.0, 0.0), 30.0, 10, 8)
    with Renderer(mesh_golden[0], ray_box=((2.5, 1.5, 4.0), (2.5, 1.5, 4.0))) as r:
        want = r.render_rays(o, d, keys, spp=4, bounces=2, seed=9)
        assert r.last_launch()["path"] == PT_PATH_WAVEFRONT
    assert same(fb, np.ascontiguousarray(cameras.rays_to_image(want, 10, 8))) and fb.max() > 0.0
    assert "wavefront path" in capsys.readouterr().out
